"""``libdaam_jointattend.so`` (include/daam_joint_attend.h) on the device, through ctypes on guarded buffers and through
``daam_amd.trace_joint(attend=True)``, held to the float64 reference of ``_joint_attend_domain`` inside the bounds derived there: every
output element, every statistic (through the probabilities it defines) and every entry of the planes formed from them, absolutely.

A query block is 128 rows, a key tile 64 keys with d = 64 and 32 with d = 128, a step 32 keys: P = 1, 5, 63, 65 sit inside one block
on either side of a step and of a d = 64 tile, 130 and 257 give two and three blocks with partial last ones; T = 1, 7, 64, 77, 154,
333 give one to three text query blocks and one to eleven text key tiles with partial last ones.  Figures of every case are printed
before they are asserted (``pytest -s``)."""
import numpy as np
import pytest
import torch

import _joint_affinity_domain as JA
import _joint_attend_domain as A
import _joint_domain as J
import _mmdit_standin as M
from test_gpu_joint_tap import DEV, GUARD, PLANE_GAP, PROMPT, _get, _guarded, _intact, _put  # noqa: F401

pytestmark = pytest.mark.gpu
ROW_GAP = 8                                           # elements between two output rows that must stay untouched
NAMES = ('qi', 'ki', 'vi', 'qt', 'kt', 'vt')


def _strides(b, h, rows, d, layout, gap=0):
    """(batch, head, row) strides in elements of a [b, h, rows, d] tensor in the layout of the projections or packed."""
    if layout == 'interleaved':
        return (rows * (h * d + gap), d, h * d + gap)
    return (h * rows * (d + gap), rows * (d + gap), d + gap)


def _image(x, dtype, layout):
    return J.bits(x.transpose(0, 2, 1, 3) if layout == 'interleaved' else x, dtype)


def _extent(shape, strides):
    return sum((n - 1) * s for n, s in zip(shape[:3], strides)) + shape[3]


def _view(flat, shape, strides):
    return np.lib.stride_tricks.as_strided(flat, shape, tuple(flat.itemsize * s for s in (*strides, 1)))


def _f32(u16, dtype):
    t = torch.from_numpy(u16.astype(np.int16).copy()).view(torch.float16 if dtype == 'f16' else torch.bfloat16)
    return t.float().numpy()


class Run:
    """One ``daam_joint_attend_forward`` on guarded buffers: inputs in ``layout``, outputs pre-filled with NaN in the same layout with
    ``ROW_GAP`` elements between rows, statistics of exactly the bytes asked for (or NULL).  Checks every guard, the gaps and that the
    inputs are unchanged; keeps the device buffers for the text kernel."""

    def __init__(self, inp, layout, with_stats=True):
        from daam_amd import _native as nat
        self.nat, self.lib = nat, nat.load_joint_attend()
        self.inp, self.dtype, self.layout = inp, inp['dtype'], layout
        b, h, P, d = inp['qi'].shape
        T = inp['kt'].shape[2]
        self.dims = (b, h, P, T, d)
        self.code = J.DAAM_F16 if self.dtype == 'f16' else J.DAAM_BF16
        self.bufs, self.strides = {}, {}
        for name in NAMES:
            im = _image(inp[name], self.dtype, layout)
            self.bufs[name] = _guarded(im.nbytes, 0)
            _put(self.bufs[name], im)
            self.strides[name] = _strides(b, h, inp[name].shape[2], d, layout)
        before = {name: self.bufs[name][0].clone() for name in NAMES}
        self.out_shape = {'oi': (b, h, P, d), 'ot': (b, h, T, d)}
        for name, rows in (('oi', P), ('ot', T)):
            self.strides[name] = _strides(b, h, rows, d, layout, ROW_GAP)
            self.bufs[name] = _guarded(2 * _extent(self.out_shape[name], self.strides[name]), 0xFF)
        self.need = self.lib.daam_joint_attend_stats_bytes(b, h, P)
        assert self.need == 8 * b * h * A.pad128(P)
        self.bufs['st'] = _guarded(self.need, 0x5A, 8) if with_stats else None
        arr = lambda names: (nat.c_int64 * (3 * len(names)))(*[v for n in names for v in self.strides[n]])
        nat.check_joint_attend(self.lib.daam_joint_attend_forward(
            *[self.ptr(n) for n in NAMES], self.ptr('oi'), self.ptr('ot'), self.code, b, h, P, T, d, arr(NAMES[:3]), arr(NAMES[3:]),
            arr(('oi', 'ot')), inp['scale'], self.ptr('st') if with_stats else None, self.need if with_stats else 0,
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert all(torch.equal(self.bufs[n][0], before[n]) for n in NAMES), 'an input changed'
        self.out = {}
        for name in ('oi', 'ot'):
            n_bytes = 2 * _extent(self.out_shape[name], self.strides[name])
            assert _intact(self.bufs[name], n_bytes), f'{name}: a guard was written'
            flat = _get(self.bufs[name], n_bytes, np.uint16, (-1,))
            self.out[name] = _view(flat, self.out_shape[name], self.strides[name]).copy()
            rest = flat.copy()
            _view(rest, self.out_shape[name], self.strides[name])[...] = 0xFFFF
            assert (rest == 0xFFFF).all(), f'{name}: the elements between two rows were written'
        self.stats = None
        if with_stats:
            assert _intact(self.bufs['st'], self.need), 'stats: a guard was written'
            self.stats = _get(self.bufs['st'], self.need, np.float32, (b * h, A.pad128(P), 2))

    def ptr(self, name):
        return self.bufs[name][0].data_ptr() + self.bufs[name][1]

    def outputs(self):
        return _f32(self.out['oi'], self.dtype), _f32(self.out['ot'], self.dtype)

    def text(self, calls, per_head, first=0):
        """``daam_joint_attend_text`` on this run's Q, text K and statistics from batch entry ``first`` on, once per ``(weight,)`` of
        ``calls`` into one guarded ``sums`` pre-filled with NaN: f32 [T, P] or [heads, T, P]."""
        b, h, P, T, d = self.dims
        planes, stride = (h, T * P + PLANE_GAP) if per_head else (1, 0)
        n_sums = 4 * ((planes - 1) * stride + T * P)
        sums = _guarded(n_sums, 0xFF, 4)
        stats_before = self.bufs['st'][0].clone()
        off = lambda name: 2 * first * self.strides[name][0]
        for n, weight in enumerate(calls):
            self.nat.check_joint_attend(self.lib.daam_joint_attend_text(
                self.ptr('qi') + off('qi'), self.ptr('kt') + off('kt'), self.ptr('st') + 8 * first * h * A.pad128(P),
                self.need - 8 * first * h * A.pad128(P), self.code, b - first, h, P, T, d, *self.strides['qi'], *self.strides['kt'],
                self.inp['scale'], weight, int(n > 0), sums[0].data_ptr() + sums[1], stride, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert _intact(sums, n_sums) and torch.equal(self.bufs['st'][0], stats_before), 'a guard or the statistics were written'
        flat = _get(sums, n_sums, np.float32, (-1,))
        if not per_head:
            return flat.reshape(T, P)
        assert all(np.isnan(flat[p * stride + T * P:(p + 1) * stride]).all() for p in range(planes - 1)), 'between two planes'
        return np.stack([flat[p * stride:p * stride + T * P].reshape(T, P) for p in range(planes)])


def _report(name, got, want, bound):
    ratio = A.worst(got, want, bound)
    print(f'\n{name}: worst error {np.abs(np.asarray(got, np.float64) - want).max():.3e}, worst device/bound {ratio:.3f}')
    return ratio


@pytest.mark.parametrize('n,case', list(enumerate(A.CASES)), ids=[A.case_id(c) for c in A.CASES])
def test_forward_statistics_and_planes_are_within_the_bounds(n, case):
    inp, layout = A.case_inputs(case), case[5]
    run = Run(inp, layout)
    again, bare = Run(inp, layout), Run(inp, layout, with_stats=False)
    for name in ('oi', 'ot'):
        assert np.array_equal(run.out[name], again.out[name]), 'a second run'
        assert np.array_equal(run.out[name], bare.out[name]), 'stats = NULL'
    assert np.array_equal(run.stats.view(np.uint32)[:, :case[0]], again.stats.view(np.uint32)[:, :case[0]]), 'a second run'
    want_i, want_t, _ = A.reference(inp)
    bound_i, bound_t = A.out_bound(inp)
    got_i, got_t = run.outputs()
    r_i = _report(f'out_img {A.case_id(case)}', got_i, want_i, bound_i)
    r_t = _report(f'out_txt {A.case_id(case)}', got_t, want_t, bound_t)
    s_bound, s_want = A.stats_bound(inp)
    r_s = _report(f'statistics {A.case_id(case)}', A.stats_probabilities(inp, run.stats), s_want, s_bound)
    per_head = bool(n % 2)
    planes = run.text([1.0], per_head)
    calls = A.tap_calls(inp)
    r_p = _report(f'text planes {A.case_id(case)}', planes, J.reference_sums(calls, per_head), J.sums_bound(calls, per_head))
    assert np.isfinite(got_i).all() and np.isfinite(got_t).all() and np.isfinite(planes).all()
    assert max(r_i, r_t, r_s, r_p) <= 1.0, (r_i, r_t, r_s, r_p)


@pytest.mark.parametrize('P,T,d,dtype,layout,per_head', [(65, 77, 64, 'f16', 'interleaved', False), (130, 154, 128, 'bf16', 'packed', True)])
def test_text_planes_chain_weights_and_the_kept_half(P, T, d, dtype, layout, per_head):
    inp = A.inputs('small', 'normal', 2, 3, P, T, d, dtype, seed=4)
    run = Run(inp, layout)
    for first in (0, 1):
        for w1, w2 in ((1.0, 1.0), (0.5, -0.25)):
            calls = A.tap_calls(inp, first, w1) + A.tap_calls(inp, first, w2)
            got = run.text([w1, w2], per_head, first)
            ratio = _report(f'two calls P={P} T={T} d={d} {dtype} first={first} weights {w1} {w2}', got, J.reference_sums(calls, per_head),
                            J.sums_bound(calls, per_head))
            assert ratio <= 1.0


@pytest.mark.parametrize('P,T,d,dtype', [(65, 77, 64, 'f16'), (130, 7, 128, 'bf16')])
def test_the_engine_feeds_the_affinity_the_forwards_statistics(P, T, d, dtype):
    """``JointAttendState.forward`` -> ``JointTapState.tap_from_stats`` and ``JointAffinityState.tap`` on the kept half: the affinity
    inside 3.26's bound, and per row text mass + image mass = slices."""
    from daam_amd import engine as E
    b, h = 2, 3
    inp = A.inputs('small', 'normal', b, h, P, T, d, dtype, seed=9)
    tdt = torch.float16 if dtype == 'f16' else torch.bfloat16
    dev = {n: torch.from_numpy(inp[n].transpose(0, 2, 1, 3).reshape(b, -1, h * d)).to(tdt).to(DEV) for n in NAMES}
    out_i, out_t, stats = E.JointAttendState().forward(*[dev[n] for n in NAMES], h, inp['scale'])
    want_i, want_t, _ = A.reference(inp)
    bound_i, bound_t = A.out_bound(inp)
    back = lambda o: o.float().cpu().numpy().reshape(b, -1, h, d).transpose(0, 2, 1, 3)
    assert _report('engine out_img', back(out_i), want_i, bound_i) <= 1.0 and _report('engine out_txt', back(out_t), want_t, bound_t) <= 1.0
    kept = stats[1 * h * A.pad128(P):]
    tap, aff = E.JointTapState(1, P, T), E.JointAffinityState(1, P)
    tap.tap_from_stats(dev['qi'][1:], dev['kt'][1:], h, inp['scale'], kept)
    aff.tap(dev['qi'][1:], dev['ki'][1:], h, inp['scale'], tap.stats)
    assert tap.stats is kept and tap.calls == aff.calls == 1 and tap.slices == aff.slices == h
    calls = A.tap_calls(inp, 1)
    planes, image = tap.sums.cpu().numpy(), aff.sums.cpu().numpy()
    assert _report('planes', planes, J.reference_sums(calls), J.sums_bound(calls)) <= 1.0
    a_bound = JA.sums_bound(calls)
    assert _report('affinity', image, JA.reference_sums(calls), a_bound) <= 1.0
    total = planes.astype(np.float64).sum(axis=0) + image.astype(np.float64).sum(axis=1)
    slack = J.sums_bound(calls).sum(axis=0) + a_bound.sum(axis=1) + (T + P) * J.U * h
    assert (np.abs(total - h) <= slack).all(), 'text mass + image mass = slices'


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
def _capture(tc):
    """Wrap ``tc.attend.forward``: every call's inputs and results as CPU tensors."""
    calls, inner = [], tc.attend.forward

    def forward(*args):
        out = inner(*args)
        calls.append(([a.detach().cpu() for a in args[:6]], args[6], args[7], out[0].cpu(), out[1].cpu(), out[2].cpu().clone()))
        return out
    tc.attend.forward = forward
    return calls


def _as_inputs(tensors, heads, scale, dtype):
    b = tensors[0].shape[0]
    split = lambda t: t.float().numpy().reshape(b, t.shape[1], heads, -1).transpose(0, 2, 1, 3)
    return dict(zip(NAMES, (split(t) for t in tensors)), scale=float(np.float32(scale)), dtype=dtype)


@pytest.mark.parametrize('dtype,size,grid', [(torch.float16, {}, (8, 8)), (torch.bfloat16, dict(height=96, width=160), (6, 10))])
def test_the_stand_in_pipeline_with_attend(dtype, size, grid):
    """Two steps of the stand-in MMDiT (blocks with and without qk norms) through ``trace_joint(attend=True, self_affinity=True)``,
    one plane and per head: every captured ``forward`` inside the bounds on ITS inputs, the final planes and the affinity inside the
    chained bounds of the captured kept halves, and the model's output no further than twice the stock processor's distance from an
    f32 run of the same stand-in."""
    import daam_amd
    steps, cells, name = 2, grid[0] * grid[1], 'f16' if dtype == torch.float16 else 'bf16'
    pipe = M.make_pipe(device=DEV, dtype=dtype, seed=3)
    pipe(PROMPT, num_inference_steps=steps, **size)
    stock = [o.float().cpu() for o in pipe.outputs]
    exact_pipe = M.make_pipe(device=DEV, dtype=torch.float32, seed=3)
    exact_pipe(PROMPT, num_inference_steps=steps, **size)
    exact = [o.float().cpu() for o in exact_pipe.outputs]
    with daam_amd.trace_joint(pipe, attend=False, **size) as tc:
        pipe(PROMPT, num_inference_steps=steps, **size)
        assert all(torch.equal(a.float().cpu(), b) for a, b in zip(pipe.outputs, stock)), 'attend=False is bit-identical'
        plain_sums = tc.state.sums.clone()
    with daam_amd.trace_joint(pipe, **size) as tc:
        pipe(PROMPT, num_inference_steps=steps, **size)
        assert torch.equal(tc.state.sums, plain_sums), 'attend=False: the planes are those of the option left out'
    for per_head in (False, True):
        recorded = M.record(pipe)
        with daam_amd.trace_joint(pipe, per_head=per_head, self_affinity=True, attend=True, **size) as tc:
            calls = _capture(tc)
            pipe(PROMPT, num_inference_steps=steps, **size)
            fused = [o.float().cpu() for o in pipe.outputs]
            sums, image, state = tc.state.sums.cpu().numpy(), tc.affinity.sums.cpu().numpy(), tc.state
        M.record(pipe, on=False)
        assert recorded == [], 'the original processor does not run on this route'
        assert len(calls) == 3 * steps and state.calls == len(calls) and state.slices == 2 * len(calls)
        taps, worst = [], 0.0
        for tensors, heads, scale, out_i, out_t, stats in calls:
            inp = _as_inputs(tensors, heads, scale, name)
            assert inp['qi'].shape == (2, 2, cells, 64) and inp['kt'].shape == (2, 2, M.CLIP_ROWS + M.T5_ROWS, 64)
            want_i, want_t, _ = A.reference(inp)
            bound_i, bound_t = A.out_bound(inp)
            back = lambda o: o.float().numpy().reshape(2, -1, heads, 64).transpose(0, 2, 1, 3)
            s_bound, s_want = A.stats_bound(inp)
            st = stats.numpy().view(np.float32).reshape(2 * heads, A.pad128(cells), 2)
            worst = max(worst, A.worst(back(out_i), want_i, bound_i), A.worst(back(out_t), want_t, bound_t),
                        A.worst(A.stats_probabilities(inp, st), s_want, s_bound))
            taps += A.tap_calls(inp, 1)
        print(f'\nstand-in {grid} {name} per_head={per_head}: worst forward / bound {worst:.3f}')
        assert worst <= 1.0
        assert _report('planes', sums, J.reference_sums(taps, per_head), J.sums_bound(taps, per_head)) <= 1.0
        assert _report('affinity', image, JA.reference_sums(taps), JA.sums_bound(taps)) <= 1.0
    for kind, dist in (('max-abs', lambda a, b: max(float((x - y).abs().max()) for x, y in zip(a, b))),
                       ('rms', lambda a, b: float(np.sqrt(np.mean([float(((x - y) ** 2).mean()) for x, y in zip(a, b)]))))):
        d_fused, d_stock = dist(fused, exact), dist(stock, exact)
        print(f'\nstand-in {grid} {name}: {kind} distance from the f32 run: fused {d_fused:.4e}, stock {d_stock:.4e}')
        assert d_fused <= 2.0 * d_stock, (kind, d_fused, d_stock)
