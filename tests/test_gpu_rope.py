"""``daam_rope_apply`` (include/daam_rope.h) on the device, through ctypes on guarded buffers and through
``engine.rope_apply``, held to the numpy oracle of ``_rope_domain`` by BIT EQUALITY: the whole memory image of every output -- the
elements a job owns and the untouched ones between them -- is compared, and a mismatch count other than zero fails.

A workgroup is 256 lanes of 8 elements: with d = 64 a head is 8 lanes, with d = 128 it is 16.  rows = 1 and 5 sit inside one workgroup
(a masked tail), 63 and 65 on either side of two, 130 with 3 heads and a batch of 2 gives 25 (d = 64) and 49 (d = 128) with a partial
last one; several jobs put job boundaries inside the grid."""
import numpy as np
import pytest
import torch

import _rope_domain as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
UNTOUCHED = 0x5A5A                                    # what the output buffers hold before a launch


def _guarded(n_bytes, fill):
    """A uint8 device buffer of ``n_bytes`` at a 16-byte aligned address between two guards of 0xA5, filled with ``fill``."""
    raw = torch.full((GUARD + 16 + n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(raw.data_ptr() + GUARD) % 16)
    raw[start:start + n_bytes] = fill
    return raw, start


def _put(buf, array):
    raw, start = buf
    flat = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1)).to(DEV)
    raw[start:start + flat.numel()] = flat


def _get(buf, n_bytes, dtype):
    raw, start = buf
    return raw[start:start + n_bytes].cpu().numpy().view(dtype).copy()


def _intact(buf, n_bytes):
    raw, start = buf
    return bool((raw[:start] == 0xA5).all()) and bool((raw[start + n_bytes:] == 0xA5).all())


_DEVICE_TABLES = {}


def _tables(d):
    """The case table of head dim ``d`` on the device, once: guarded cos and sin buffers."""
    if d not in _DEVICE_TABLES:
        bufs = []
        for t in R.case_table(d):
            buf = _guarded(t.nbytes, 0)
            _put(buf, t)
            bufs.append((buf, t.nbytes, buf[0].clone()))
        _DEVICE_TABLES[d] = bufs
    return _DEVICE_TABLES[d]


def apply_raw(specs, dtype, d):
    """One ``daam_rope_apply`` of the jobs ``specs`` = ``(x f32 [b, rows, heads, d], layout of x, layout of out, first table row)``:
    the memory image of every job's output (uint16, pre-filled with ``UNTOUCHED``), after checking every guard and that x and the
    tables are unchanged."""
    from daam_amd import _native as nat
    lib = nat.load_rope()
    tables = _tables(d)
    jobs, held = (nat.RopeJob * len(specs))(), []
    for n, (x, x_layout, out_layout, first_row) in enumerate(specs):
        b, rows, heads, _ = x.shape
        xs, os_ = R.strides_of(x_layout, rows, heads, d), R.strides_of(out_layout, rows, heads, d)
        image = R.place(R.bits(x, dtype), xs, fill=0x7E7E)            # a NaN pattern in both dtypes between the rows of a gapped x
        xb, ob = _guarded(image.nbytes, 0), _guarded(2 * R.extent(x.shape, os_), 0x5A)
        _put(xb, image)
        held.append((xb, image.nbytes, xb[0].clone(), ob, 2 * R.extent(x.shape, os_)))
        ptr = lambda buf: buf[0].data_ptr() + buf[1]
        cos, sin = (ptr(t[0]) + 4 * first_row * d for t in tables)
        jobs[n] = nat.RopeJob(ptr(xb), ptr(ob), cos, sin, b, heads, rows, *xs, *os_, d)
    nat.check_rope(lib.daam_rope_apply(jobs, len(specs), R.DAAM_F16 if dtype == 'f16' else R.DAAM_BF16, d, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for buf, n_bytes, before in tables:
        assert _intact(buf, n_bytes) and torch.equal(buf[0], before), 'a table changed'
    out = []
    for xb, x_bytes, before, ob, o_bytes in held:
        assert _intact(xb, x_bytes) and torch.equal(xb[0], before), 'an input changed'
        assert _intact(ob, o_bytes), 'a guard of out was written'
        out.append(_get(ob, o_bytes, np.uint16))
    return out


def expected(spec, dtype, d):
    x, _, out_layout, first_row = spec
    cos, sin = R.case_table(d)
    return R.place(R.rotate(x, cos, sin, dtype, first_row), R.strides_of(out_layout, x.shape[1], x.shape[2], d), fill=UNTOUCHED)


def _hold(name, got, want):
    wrong = int((got != want).sum())
    print(f'\n{name}: {got.size} uint16 of the output image, {wrong} differ from the oracle')
    assert got.shape == want.shape and wrong == 0, f'{name}: {wrong} of {got.size} differ'


@pytest.mark.parametrize('case', R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_one_job_is_bit_equal_to_the_oracle(case):
    rows, heads, batch, d, dtype, x_layout, out_layout, first_row, regime = case
    x, _, _ = R.case_inputs(case)
    spec = (x, x_layout, out_layout, first_row)
    got, = apply_raw([spec], dtype, d)
    again, = apply_raw([spec], dtype, d)
    assert np.array_equal(got, again), 'a second run'
    _hold(R.case_id(case), got, expected(spec, dtype, d))


JOB_SETS = {
    3: [(130, 3, 2, 'interleaved', 'gapped', 24, 'normal'), (65, 3, 1, 'packed', 'interleaved', 24, 'large'), (5, 1, 2, 'gapped', 'packed', 0, 'subnormal')],
    4: [(1, 3, 1, 'interleaved', 'interleaved', 30, 'normal'), (63, 1, 2, 'gapped', 'gapped', 24, 'large'), (130, 3, 1, 'packed', 'packed', 0, 'normal'),
        (5, 3, 2, 'interleaved', 'packed', 100, 'subnormal')],
}


@pytest.mark.parametrize('d', R.HEAD_DIMS)
@pytest.mark.parametrize('dtype', ['f16', 'bf16'])
@pytest.mark.parametrize('n_jobs', sorted(JOB_SETS))
def test_several_jobs_of_different_sizes_in_one_launch(n_jobs, dtype, d):
    specs = [(R.inputs(regime, batch, rows, heads, d, dtype, seed=n_jobs + n), x_layout, out_layout, first_row)
             for n, (rows, heads, batch, x_layout, out_layout, first_row, regime) in enumerate(JOB_SETS[n_jobs])]
    got = apply_raw(specs, dtype, d)
    again = apply_raw(specs, dtype, d)
    for n, spec in enumerate(specs):
        assert np.array_equal(got[n], again[n]), 'a second run'
        _hold(f'{n_jobs} jobs, {dtype}, d {d}, job {n}', got[n], expected(spec, dtype, d))
        alone, = apply_raw([spec], dtype, d)
        assert np.array_equal(alone, got[n]), 'a job gives the same bits alone and among others'


@pytest.mark.parametrize('dtype,d', [('f16', 64), ('bf16', 128)])
def test_what_lies_between_rows_and_heads_is_untouched(dtype, d):
    x = R.inputs('normal', 2, 65, 3, d, dtype, seed=9)
    spec = (x, 'interleaved', 'gapped', 24)
    got, = apply_raw([spec], dtype, d)
    strides = R.strides_of('gapped', 65, 3, d)
    owned = R.place(np.ones(x.shape, np.uint16), strides, fill=0).astype(bool)
    assert (~owned).sum() == 2 * 65 * (3 * 8 + 16) - 16 and (got[~owned] == UNTOUCHED).all(), 'an element no job owns was written'
    _hold(f'gapped out {dtype} d {d}', got, expected(spec, dtype, d))


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,d,layout', [(torch.float16, 64, 'rows'), (torch.bfloat16, 128, 'columns')])
def test_the_engine_launcher_on_the_jobs_of_a_double_stream_call(dtype, d, layout):
    """Three jobs into one buffer as ``trace_flux`` lays them out (text K, image K, Q), strides read off the tensors, the table through
    ``RopeTable``: bit-equal to the oracle and to torch eager on the same GPU."""
    from daam_amd import engine as E
    import _flux_standin as FS
    name = 'f16' if dtype == torch.float16 else 'bf16'
    T, (h, w), heads = R.TEXT_ROWS, R.GRID, 3
    P = h * w
    cos_np, sin_np = R.case_table(d)
    cos, sin = (torch.from_numpy(t).to(DEV) for t in (cos_np, sin_np))
    if layout == 'columns':
        cos, sin = (t.t().contiguous().t() for t in (cos, sin))
    xs = {key: R.inputs('normal', 1, rows, heads, d, name, seed=n) for n, (key, rows) in enumerate((('q', P), ('k_img', P), ('k_txt', T)))}
    dev = {key: torch.from_numpy(v.reshape(1, v.shape[1], heads * d)).to(DEV).to(dtype) for key, v in xs.items()}
    table = E.RopeTable()
    c, s = table.get(cos), table.get(sin)
    assert len(table) == (2 if layout == 'columns' else 0) and table.get(cos) is c
    buf = torch.full((1, T + 2 * P, heads * d), float('nan'), dtype=dtype, device=DEV)
    E.rope_apply([(dev['q'], buf[:, T + P:], c[T:], s[T:], heads), (dev['k_img'], buf[:, T:T + P], c[T:], s[T:], heads),
                  (dev['k_txt'], buf[:, :T], c[:T], s[:T], heads)], d)
    got = buf.view(torch.int16).cpu().numpy().view(np.uint16).reshape(T + 2 * P, heads, d)
    for key, rows, first_row in (('k_txt', slice(0, T), 0), ('k_img', slice(T, T + P), T), ('q', slice(T + P, T + 2 * P), T)):
        want = R.rotate(xs[key], cos_np, sin_np, name, first_row)[0]
        _hold(f'engine {key} {name} d {d}', got[rows], want)
        eager = FS.apply_rotary(dev[key].view(1, -1, heads, d).transpose(1, 2), cos[first_row:first_row + want.shape[0]],
                                sin[first_row:first_row + want.shape[0]]).transpose(1, 2)
        assert np.array_equal(eager.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)[0], want), 'torch eager on the GPU gives these bits'
    with pytest.raises(ValueError, match='RopeTable.get'):
        E.rope_apply([(dev['q'], buf[:, T + P:], cos[T:].double(), sin[T:].double(), heads)], d)
    with pytest.raises(E.nat.DaamError, match='overlaps'):
        E.rope_apply([(dev['q'], dev['q'], c[T:], s[T:], heads)], d)
