"""``daam_finalize_bins`` -- ``finalize_bin_sum_kernel`` and the host planner around it -- token row by token row against float64, through
the raw ABI on buffers of ours: cut pieces and unaligned keys, 2 / 7 / 50 windows up to 2^20 apart, the planner's branches, the
scratch's life and the task table's limit.  Planes, reference, bound and the emulation's footing: ``tests/_bins_domain.py`` and
``tests/test_bins_domain_cpu.py``.  Every case asserts through ``daam_last_kernels(ctx, 1, ...)`` which kernels ran and that every
window buffer is bit-identical afterwards.

Where outputs are compared bit for bit (two calls of the same work), every output element receives at most two atomic adds -- one x2 key
and one same-size key per group, or one launch per class of one key each -- and ``(0 + a) + b == (0 + b) + a`` in f32.

What an MI355X gave is in LABNOTES.md (R8.11); run with ``-s``, every case prints ``BINDOMAIN`` lines with its figures.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import _bins_domain as bd
import _finalize_domain as fd

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = -7.0
I32 = ctypes.c_int32


def expected_kernels(sides, out_side, tag, keys_per_side=None):
    """``(names of the grouped class kernels over layers of ``sides`` on planes of dtype ``tag``, does an MFMA x2 kernel run)``: the planner's
    rules (fin_plan) restated.  ``keys_per_side``: selected keys of a group per side (default: one each) for the folding rule."""
    n = keys_per_side or {s: 1 for s in sides}
    names, mfma = set(), False
    fold = out_side == 64 and 32 in sides and 64 in sides and n[64] <= 2 * n[32]
    for side in sides:
        if out_side == 64 and side == 32:
            names.add(f'finalize_up32_pipe_grouped_kernel<{tag}' + (' + same-size keys>' if fold else '>'))
            mfma = True
        elif side == out_side and (side * side) % 8 == 0:
            if not fold:
                names.add(f'finalize_same_grouped_kernel<{tag}>')
        elif out_side == 64 and side == 16:
            names.add(f'finalize_up_grouped_kernel<16><{tag}>')
        elif out_side == 64 and side == 128:
            names.add(f'finalize_down2_grouped_kernel<{tag}>')
        else:
            names.add(f'finalize_grouped_kernel<{tag}>')
    return names, mfma


class Binned:
    """A time-binned native context over buffers of ours: layer l holds ``planes[l]`` = ``[nb, heads, 77, hw]`` in the sums' dtype,
    ``offset`` elements behind a 16-byte boundary."""

    def __init__(self, sides, heads, out_side, dtype, planes, offset=0):
        from daam_amd import _native as nat
        self.nat, self.lib = nat, nat.load()
        self.sides, self.heads, self.out_side, self.dtype, self.planes = tuple(sides), heads, out_side, dtype, planes
        self.nb = planes[0].shape[0]
        self.keys = bd.key_table(sides, heads)
        self.plane = bd.TOKENS * out_side * out_side
        self.stream = torch.cuda.current_stream().cuda_stream
        code = {'float16': nat.DAAM_F16, 'bfloat16': nat.DAAM_BF16, 'float32': nat.DAAM_F32}[dtype]
        tdt = {'float16': torch.float16, 'bfloat16': torch.bfloat16, 'float32': torch.float32}[dtype]
        self.ctx = nat.c_void_p()
        nat.check(self.lib.daam_ctx_create(len(sides), bd.TOKENS, out_side, code, nat.byref(self.ctx)))
        nat.check(self.lib.daam_ctx_set_time_bins(self.ctx, self.nb, (I32 * self.nb)(*range(self.nb))))
        self.bufs, self.views, self.addrs = [], [], []
        for layer, (side, p) in enumerate(zip(sides, planes)):
            assert p.shape == (self.nb, heads, bd.TOKENS, side * side)
            buf = torch.zeros(p.size + 64, dtype=tdt, device=DEV)               # room for the offset; the tail stays zero
            assert buf.data_ptr() % 16 == 0
            view = buf[offset:offset + p.size]
            view.copy_(torch.from_numpy(np.ascontiguousarray(p).reshape(-1)).to(DEV).to(tdt))
            assert view.data_ptr() == buf.data_ptr() + offset * bd.ELEM[dtype]
            nat.check(self.lib.daam_layer_configure(self.ctx, layer, heads, side, out_side // side if side <= out_side else 0, view.data_ptr()))
            self.bufs.append(buf)
            self.views.append(view)
            self.addrs.append(view.data_ptr())
        self.before = [b.clone() for b in self.bufs]

    def close(self):
        if self.ctx is not None:
            self.lib.daam_ctx_destroy(self.ctx)
            self.ctx = None

    def last_kernels(self):
        buf = ctypes.create_string_buffer(4096)
        self.nat.check(self.lib.daam_last_kernels(self.ctx, 1, buf, len(buf)))
        return buf.value.decode()

    def launched(self):
        names = self.last_kernels()
        return set(re.split(r'\+(?![^<]*>)', names)) if names else set()

    def call(self, key_set, groups, with_sets=True):
        """``daam_finalize_bins`` over ``groups`` = ``[(set, b0, b1, rows)]``: ``(status, [n, 77, out, out] numpy, launched names)``."""
        n = len(groups)
        out = torch.full((n, bd.TOKENS, self.out_side, self.out_side), SENTINEL, device=DEV)
        rc = self.lib.daam_finalize_bins(self.ctx, (I32 * len(key_set))(*key_set), n,
                                         (I32 * n)(*[g[0] for g in groups]) if with_sets else None,
                                         (I32 * n)(*[g[1] for g in groups]), (I32 * n)(*[g[2] for g in groups]),
                                         (I32 * n)(*[g[3] for g in groups]), out.data_ptr(), self.plane, self.stream)
        torch.cuda.synchronize()
        return rc, out.cpu().numpy(), self.launched()

    def untouched(self):
        return all(torch.equal(a, b) for a, b in zip(self.bufs, self.before))

    def keys_of(self, key_set, st):
        return [k for k, s in zip(self.keys, key_set) if s == st]

    def branches(self, key_set, groups):
        """Branches of the reduction the call's tasks take, from the real addresses (empty: the call runs no reduction)."""
        got = set()
        for st, b0, b1, rows in groups:
            got |= bd.branches(self.sides, self.heads, self.dtype, self.addrs, self.keys_of(key_set, st), b0, b1, rows)
        return got

    def hold(self, what, key_set, groups, kind, got, names, reduced, want_cache=None):
        """Every group of a finished call against the bound, the rows beyond its crop against the sentinel, the kernels by name."""
        sel_sides = sorted({self.sides[l] for st, *_ in groups for l, _ in self.keys_of(key_set, st)})
        per_side = {s: min(sum(1 for l, _ in self.keys_of(key_set, st) if self.sides[l] == s) for st, *_ in groups) for s in sel_sides}
        tag = 'f32' if reduced else bd.TAG[self.dtype]
        want_names, mfma = expected_kernels(sel_sides, self.out_side, tag, per_side)
        if reduced:
            want_names = want_names | {f'finalize_bin_sum_kernel<{bd.TAG[self.dtype]}>'}
        assert names == want_names, (what, names, want_names)
        assert self.untouched(), f'{what}: a window buffer changed'
        worst = rel = 0.0
        for gi, (st, b0, b1, rows) in enumerate(groups):
            ck = (st, b0, b1)
            if want_cache is not None and ck in want_cache:
                want, allowance, exact = want_cache[ck]
            else:
                want, allowance, exact = bd.reference(self.planes, self.sides, self.out_side, self.keys_of(key_set, st), b0, b1,
                                                      bd.TOKENS if want_cache is not None else rows)
                if want_cache is not None:
                    want_cache[ck] = (want, allowance, exact)
            if kind == 'exact':
                assert exact, f'{what}: the f32 sum of exact planes is not exact'
            if kind == 'exact' or b1 - b0 == 1:
                allowance = 0 * allowance
            r, q = bd.check(got[gi, :rows], want[:rows], allowance[:rows], mfma, f'{what} group {gi} {groups[gi]}')
            worst, rel = max(worst, r), max(rel, q)
            assert (got[gi, rows:] == SENTINEL).all(), f'{what} group {gi}: rows beyond the crop written'
        bd.report(what, names, self.branches(key_set, groups) if reduced else set(), worst, rel)


@pytest.mark.parametrize('dtype', bd.DTYPES)
@pytest.mark.parametrize('name', list(bd.CUT_SETS))
def test_cut_pieces(name, dtype):
    """Window range [0, 3) at rows 1, 5 and 77 (one call of three groups) on every cut-piece set, levelled / signed / exact planes.  The
    branches the set is there for are computed from the buffers' addresses and asserted before anything runs.  The ABI documents no
    alignment for ``acc``: the set one element off a 16-byte boundary must simply work."""
    spec = bd.CUT_SETS[name]
    total = len(spec['sides']) * spec['heads']
    groups = [(0, 0, bd.CUT_NB, rows) for rows in bd.ROWS]
    for kind in bd.KINDS:
        planes = bd.native_windows(spec['sides'], kind, bd.CUT_NB, spec['heads'], dtype)
        c = Binned(spec['sides'], spec['heads'], spec['out_side'], dtype, planes, spec['offset'])
        try:
            for g in groups:
                assert c.branches([0] * total, [g]) == spec['reaches'][bd.ELEM[dtype]], (name, dtype, g, c.branches([0] * total, [g]))
            rc, got, names = c.call([0] * total, groups)
            assert rc == 0, c.lib.daam_last_error()
            c.hold(f'cut {name} {dtype} {kind}', [0] * total, groups, kind, got, names, reduced=True)
        finally:
            c.close()


@pytest.mark.parametrize('dtype', bd.DTYPES)
@pytest.mark.parametrize('kind', bd.KINDS)
def test_window_count(kind, dtype):
    """2, 7 and 50 windows of a 50-window context, sides 32 + 64, in one call: the f32 scratch planes take the grouped pipelined MFMA
    kernel with the same-size key folded in, asserted by name."""
    planes = bd.native_windows(bd.COUNT_SIDES, kind, bd.COUNT_NB, bd.COUNT_HEADS, dtype)
    assert sum(float(np.abs(p.astype(np.float64)).sum(0).max()) for p in planes) <= fd.DOMAIN_MAX
    c = Binned(bd.COUNT_SIDES, bd.COUNT_HEADS, 64, dtype, planes)
    try:
        groups = [(0, b0, b1, bd.TOKENS) for b0, b1 in bd.COUNT_RANGES]
        rc, got, names = c.call([0, 0], groups)
        assert rc == 0, c.lib.daam_last_error()
        assert names == {f'finalize_bin_sum_kernel<{bd.TAG[dtype]}>', 'finalize_up32_pipe_grouped_kernel<f32 + same-size keys>'}, names
        c.hold(f'count {kind} {dtype}', [0, 0], groups, kind, got, names, reduced=True)
    finally:
        c.close()


PLAN_SIDES, PLAN_HEADS, PLAN_NB = (16, 32, 64), 2, 4


@pytest.mark.parametrize('dtype', bd.DTYPES)
def test_planner(dtype):
    """One call each: the same (set, window) twice (forces the reduction on single windows), a single window beside a range, overlapping
    ranges over two sets, two sets on the direct path, 64 groups.  Two sets: even / odd keys, so each set has one key per layer."""
    planes = bd.native_windows(PLAN_SIDES, 'signed', PLAN_NB, PLAN_HEADS, dtype, seed=1)
    exact = bd.native_windows(PLAN_SIDES, 'exact', PLAN_NB, PLAN_HEADS, dtype, seed=1)
    total = len(PLAN_SIDES) * PLAN_HEADS
    one, two = [0] * total, [k % 2 for k in range(total)]
    ranges = [(b0, b1) for b0 in range(PLAN_NB) for b1 in range(b0 + 1, PLAN_NB + 1)]
    many = [(g % 2, *ranges[g % len(ranges)], 1 + (7 * g) % 23) for g in range(64)]
    cases = [
        ('same window twice', one, [(0, 1, 2, 77), (0, 1, 2, 30)], True),
        ('single beside range', one, [(0, 0, 1, 77), (0, 0, 3, 40)], True),
        ('overlapping ranges', two, [(0, 0, 2, 77), (0, 1, 3, 77), (1, 0, 4, 20), (1, 2, 4, 33)], True),
        ('two sets direct', two, [(0, 0, 1, 77), (1, 0, 1, 9), (0, 2, 3, 40), (1, 1, 2, 77)], False),
        ('64 groups', two, many, True),
    ]
    for kind, data in (('signed', planes), ('exact', exact)):
        c = Binned(PLAN_SIDES, PLAN_HEADS, 64, dtype, data)
        cache = {}
        try:
            for what, key_set, groups, reduced in cases:
                rc, got, names = c.call(key_set, groups)
                assert rc == 0, c.lib.daam_last_error()
                assert ('finalize_bin_sum_kernel<%s>' % bd.TAG[dtype] in names) == reduced, (what, names)
                c.hold(f'planner {what} {dtype} {kind}', key_set, groups, kind, got, names, reduced, cache if key_set is two else None)
        finally:
            c.close()


@pytest.mark.parametrize('dtype', bd.DTYPES)
def test_whole_generation_entry_points_are_the_explicit_range(dtype):
    """``daam_finalize`` and ``daam_finalize_groups`` on a binned context = ``daam_finalize_bins`` over [0, nb), bit for bit (one x2 and one
    same-size key per group: see the module docstring)."""
    sides, heads, nb = (32, 64), 2, 3
    planes = bd.native_windows(sides, 'signed', nb, heads, dtype, seed=2)
    c = Binned(sides, heads, 64, dtype, planes)
    try:
        two = [k % 2 for k in range(4)]
        rc, want, names = c.call(two, [(0, 0, nb, 77), (1, 0, nb, 40)], with_sets=False)
        assert rc == 0, c.lib.daam_last_error()
        c.hold(f'entry points, explicit range {dtype}', two, [(0, 0, nb, 77), (1, 0, nb, 40)], 'signed', want, names, True)
        out = torch.full((2, 77, 64, 64), SENTINEL, device=DEV)
        c.nat.check(c.lib.daam_finalize_groups(c.ctx, (I32 * 4)(*two), 2, (I32 * 2)(77, 40), out.data_ptr(), c.plane, c.stream))
        torch.cuda.synchronize()
        assert c.launched() == names and np.array_equal(out.cpu().numpy(), want)
        one = torch.full((77, 64, 64), SENTINEL, device=DEV)
        c.nat.check(c.lib.daam_finalize(c.ctx, (ctypes.c_uint8 * 4)(1, 0, 1, 0), 77, one.data_ptr(), c.stream))
        torch.cuda.synchronize()
        assert c.launched() == names and np.array_equal(one.cpu().numpy(), want[0])
        assert c.untouched()
    finally:
        c.close()


@pytest.mark.parametrize('dtype', bd.DTYPES)
def test_scratch_life(dtype):
    """A small call, a larger one that regrows the scratch, the small one again on the grown scratch: all three inside the bound, the
    first and the third bit-identical (two keys per group)."""
    sides, heads, nb = (32, 64), 1, 3
    planes = bd.native_windows(sides, 'levelled', nb, heads, dtype, seed=3)
    c = Binned(sides, heads, 64, dtype, planes)
    try:
        small = [(0, 0, 2, 5)]
        large = [(0, b0, b1, 77) for b0, b1 in [(0, 3), (1, 3), (0, 2), (0, 3), (1, 3), (0, 2), (0, 3), (1, 3)]]
        outs = []
        for what, groups in (('small', small), ('large', large), ('small again', small)):
            rc, got, names = c.call([0, 0], groups)
            assert rc == 0, c.lib.daam_last_error()
            c.hold(f'scratch {what} {dtype}', [0, 0], groups, 'levelled', got, names, True)
            outs.append(got)
        assert np.array_equal(outs[0], outs[2])
    finally:
        c.close()


def test_engine_splits_seventy_groups():
    """``engine.time_heat_maps`` with 70 groups: two ABI calls (64 + 6) on one scratch.  Eight one-step windows of two prompts, fp16."""
    import test_gpu_finalize_domain as tfd
    sides, nb, dtype = (32, 64), 8, 'float16'
    steps = []
    for b in range(nb):
        base = fd.draw_planes(sides, 'nonneg', heads=4, seed=40 + b)
        steps.append([fd.round_to(p * np.float32(bd.window_scale(b)), dtype) for p in base])
    eng = tfd._engine(sides, dtype, time_bins=list(range(nb)))
    try:
        for planes in steps:                                                    # step s of every layer lands in window s
            tfd._tap(eng, planes, sides, dtype)
        ranges = [(b0, b1) for b0 in range(nb) for b1 in range(b0 + 1, nb + 1)]
        groups = [(b0, b1, p) for p in range(2) for b0, b1 in ranges][:70]
        n_rows = [77, 30]
        got = eng.time_heat_maps(groups, 2, n_rows).cpu().numpy()
        assert tfd._launched(eng) == {'finalize_bin_sum_kernel<f16>', 'finalize_up32_pipe_grouped_kernel<f32 + same-size keys>'}
        # the library's layout of the kept half, prompt p = kept heads [2p, 2p + 2)
        native = bd.native([np.stack([steps[b][l] for b in range(nb)]) for l in range(len(sides))])
        worst = rel = 0.0
        for gi, (b0, b1, p) in enumerate(groups):
            keys = [(l, h) for l in range(len(sides)) for h in (2 * p, 2 * p + 1)]
            want, allowance, _ = bd.reference(native, sides, 64, keys, b0, b1, n_rows[p])
            r, q = bd.check(got[gi, :n_rows[p]], want, allowance, True, f'engine group {gi} {groups[gi]}')
            worst, rel = max(worst, r), max(rel, q)
        bd.report('engine 70 groups float16', tfd._launched(eng), {'pieces'}, worst, rel)
    finally:
        eng.close()


def test_task_table_limit():
    """64 range groups over 2800 keys of side 2 are 179 200 tasks of 48 bytes, more than the 8 MiB ring holds: DAAM_E_UNSUPPORTED, nothing
    launched, the output untouched; a smaller call on the same context is served afterwards."""
    sides, heads, nb, dtype = (2,), 2800, 2, 'float16'
    rng = np.random.default_rng(5)
    planes = [np.exp(rng.standard_normal((nb, heads, bd.TOKENS, 4))).astype(np.float16)]
    c = Binned(sides, heads, 64, dtype, planes)
    try:
        assert c.last_kernels() == ''
        rc, got, names = c.call([0] * heads, [(0, 0, 2, 1)] * 64)
        assert rc == c.nat.E_UNSUPPORTED, rc
        assert names == set() and (got == SENTINEL).all() and c.untouched()
        few = [0 if k in (0, 1, 1399, 2799) else -1 for k in range(heads)]
        groups = [(0, 0, 2, 77), (0, 1, 2, 5)]
        rc, got, names = c.call(few, groups)
        assert rc == 0, c.lib.daam_last_error()
        c.hold('limit: smaller call afterwards', few, groups, 'levelled', got, names, True)
    finally:
        c.close()
