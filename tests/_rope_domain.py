"""Shared by ``test_rope_cpu.py`` and ``test_gpu_rope.py``: the rotary pass (include/daam_rope.h) as a numpy f32 oracle,
operation by operation as the header specifies it, the torch CPU expression it has to equal bit for bit, the real FLUX tables, the
inputs of the cases, memory images of the layouts, and the mutants that show a bit-equality check can fail.  Test-only.

Values are f32 arrays x [batch, rows, heads, d] exactly representable in the case's dtype ('f16' or 'bf16'); results are uint16 arrays
of the same shape: the device representation.  There is no tolerance anywhere: every comparison is of bits.
"""
import numpy as np
import torch

from _self_affinity_domain import bits, quantize

F32, F64 = np.float32, np.float64
DAAM_F16, DAAM_BF16 = 0, 2
E_INVALID = -1
AXES = {64: (16, 24, 24), 128: (16, 56, 56)}          # FLUX's axes_dims_rope; head dim 64 with the same split in proportion
THETA = 10000.0
TEXT_ROWS, GRID = 19, (12, 12)                        # the table of the cases: 19 text rows, then 144 image rows
REGIMES = ('normal', 'subnormal', 'large')
TORCH = {'f16': torch.float16, 'bf16': torch.bfloat16}


# ---- tables --------------------------------------------------------------------------------------------------------------------------
def flux_table(text_rows, h, w, d):
    """``(cos, sin)`` f32 [text_rows + h w, d] as FLUX builds them: ids (0, 0, 0) for the text rows and (0, y, x) for the image rows;
    per axis the angles pos / theta^(2 i / dim) in float64, cast to f32, every value twice (interleaved pairs)."""
    ids = np.zeros((text_rows + h * w, 3), F64)
    ids[text_rows:, 1] = np.repeat(np.arange(h), w)
    ids[text_rows:, 2] = np.tile(np.arange(w), h)
    cos, sin = [], []
    for axis, dim in enumerate(AXES[d]):
        omega = 1.0 / THETA ** (np.arange(0, dim, 2, dtype=F64) / dim)
        angles = np.outer(ids[:, axis], omega)
        cos.append(np.repeat(np.cos(angles).astype(F32), 2, axis=1))
        sin.append(np.repeat(np.sin(angles).astype(F32), 2, axis=1))
    return np.ascontiguousarray(np.concatenate(cos, axis=1)), np.ascontiguousarray(np.concatenate(sin, axis=1))


_TABLES = {}


def case_table(d):
    if d not in _TABLES:
        _TABLES[d] = flux_table(TEXT_ROWS, *GRID, d)
    return _TABLES[d]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def inputs(regime, batch, rows, heads, d, dtype, seed=0):
    """f32 [batch, rows, heads, d], every value finite and exact in ``dtype``: N(0, 1); subnormals of the dtype (whole multiples of
    its smallest one, below its smallest normal); |x| up to 0.9 of the dtype's maximum, so that a rotated pair can round to +-inf."""
    rng = np.random.default_rng(seed * 7919 + rows * 131 + heads * 17 + d + batch)
    shape = (batch, rows, heads, d)
    if regime == 'normal':
        x = quantize(rng.standard_normal(shape), dtype)
    elif regime == 'subnormal':
        unit, top = (2.0 ** -24, 700) if dtype == 'f16' else (2.0 ** -133, 88)          # a rotated pair (x sqrt 2) stays subnormal
        x = (rng.integers(-top, top + 1, shape).astype(F64) * unit).astype(F32)
    else:
        top = 65504.0 if dtype == 'f16' else float(torch.finfo(torch.bfloat16).max)
        x = quantize(rng.uniform(-0.9, 0.9, shape) * top, dtype)
    assert np.isfinite(x).all() and np.array_equal(quantize(x, dtype), x)
    return x


ROWS, HEADS, BATCHES, HEAD_DIMS, LAYOUTS, OFFSETS = (1, 5, 63, 65, 130), (1, 3), (1, 2), (64, 128), ('interleaved', 'packed'), (0, 24)


def _case(ri, rows, di, d, ti, dtype, gi, regime):
    n = ri + di + ti + gi
    return (rows, HEADS[(n + ri // 2) % 2], BATCHES[(n // 2 + di) % 2], d, dtype, LAYOUTS[(ri + gi) % 2], LAYOUTS[(ri + gi + di + ti // 1 + ri // 2) % 2],
            OFFSETS[(n + gi // 2) % 2], regime)


# (rows, heads, batch, d, dtype, layout of x, layout of out, first table row, regime): every rows x head dim x dtype x regime; the
# head counts, batches, layouts and table offsets rotate so that each value meets every head dim, both dtypes and every regime.
CASES = [_case(ri, rows, di, d, ti, dtype, gi, regime) for ri, rows in enumerate(ROWS) for di, d in enumerate(HEAD_DIMS)
         for ti, dtype in enumerate(('f16', 'bf16')) for gi, regime in enumerate(REGIMES)]


def case_id(c):
    return f'r{c[0]}-h{c[1]}-b{c[2]}-d{c[3]}-{c[4]}-{c[5]}-to-{c[6]}-row{c[7]}-{c[8]}'


def case_inputs(c):
    """``(x, cos table, sin table)`` of a case; the case reads table rows [c[7], c[7] + rows)."""
    rows, heads, batch, d, dtype = c[:5]
    return (inputs(c[8], batch, rows, heads, d, dtype, seed=rows + d),) + case_table(d)


# ---- rounding ------------------------------------------------------------------------------------------------------------------------
def round_bits(v, dtype):
    """uint16: f32 values rounded to nearest, ties to even, by torch CPU's ``.to(dtype)``."""
    return bits(v, dtype)


def truncate_bits(v, dtype):
    """uint16: f32 values rounded TOWARDS ZERO (the mutant).  Where the nearest value lies further from zero than ``v``, the value
    one step closer to zero: in these sign-magnitude formats that is the bit pattern minus one."""
    near = bits(v, dtype)
    back = torch.from_numpy(near.view(np.int16).copy()).view(TORCH[dtype]).float().numpy()
    with np.errstate(invalid='ignore'):
        beyond = np.abs(back.astype(F64)) > np.abs(np.asarray(v, F64))
    return np.where(beyond, near - 1, near).astype(np.uint16)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def rotate(x, cos, sin, dtype, first_row=0, mutant=None):
    """uint16 [batch, rows, heads, d]: the header's arithmetic in numpy f32 -- four products, two sums per pair, each one IEEE f32
    operation (numpy fuses nothing), then one rounding.  ``cos`` / ``sin``: the whole table; the job reads rows from ``first_row``.
    ``mutant``: one of ``MUTANTS``."""
    b, rows, heads, d = x.shape
    x = np.asarray(x, F32)
    if mutant == 'no_row_offset':
        first_row = 0
    if mutant == 'head_as_row':                       # element (r, h) fetched at r * row_stride + h * row_stride
        r, h = np.meshgrid(np.arange(rows), np.arange(heads), indexing='ij')
        x = x[:, (r + h) % rows, 0]
    c = np.asarray(cos, F32)[first_row:first_row + rows][None, :, None, :]
    s = np.asarray(sin, F32)[first_row:first_row + rows][None, :, None, :]
    assert c.shape[1] == rows
    if mutant == 'sin_sign':
        s = -s
    with np.errstate(over='ignore', invalid='ignore'):
        if mutant == 'half_split':                    # use_real_unbind_dim=-2: element c pairs with c +- d / 2
            lo, hi = x[..., :d // 2], x[..., d // 2:]
            turned = np.concatenate([-hi, lo], axis=-1)
            out = (x * c).astype(F32) + (turned * s).astype(F32)
        else:
            even, odd = x[..., 0::2], x[..., 1::2]
            out = np.empty_like(x)
            out[..., 0::2] = (even * c[..., 0::2]).astype(F32) + ((-odd) * s[..., 0::2]).astype(F32)
            out[..., 1::2] = (odd * c[..., 1::2]).astype(F32) + (even * s[..., 1::2]).astype(F32)
    assert out.dtype == F32
    return (truncate_bits if mutant == 'truncate' else round_bits)(out, dtype)


MUTANTS = ('half_split', 'sin_sign', 'no_row_offset', 'head_as_row', 'truncate')


def torch_expression(x, cos, sin, dtype, first_row=0):
    """uint16: ``(x.float() * cos + x_rotated.float() * sin).to(x.dtype)`` on the CPU, as diffusers' ``apply_rotary_emb`` writes it
    (``use_real=True, use_real_unbind_dim=-1``)."""
    rows = x.shape[1]
    t = torch.from_numpy(np.ascontiguousarray(x, F32)).to(TORCH[dtype])
    c = torch.from_numpy(np.ascontiguousarray(cos[first_row:first_row + rows]))[None, :, None, :]
    s = torch.from_numpy(np.ascontiguousarray(sin[first_row:first_row + rows]))[None, :, None, :]
    real, imag = t.reshape(*t.shape[:-1], -1, 2).unbind(-1)
    turned = torch.stack([-imag, real], dim=-1).flatten(3)
    out = (t.float() * c + turned.float() * s).to(t.dtype)
    return out.view(torch.int16).numpy().view(np.uint16)


# ---- memory images -------------------------------------------------------------------------------------------------------------------
def strides_of(layout, rows, heads, d):
    """``(stride_b, stride_r, stride_h)`` in elements: what the projections give ('interleaved', [b, rows, heads d]), a packed
    [b, heads, rows, d], or 'gapped': the interleaved order with 8 unused elements behind every head and 16 more behind every row."""
    if layout == 'interleaved':
        return rows * heads * d, heads * d, d
    if layout == 'packed':
        return heads * rows * d, d, rows * d
    row = heads * (d + 8) + 16
    return rows * row + 8, row, d + 8


def extent(shape, strides):
    b, rows, heads, d = shape
    return (b - 1) * strides[0] + (rows - 1) * strides[1] + (heads - 1) * strides[2] + d


def place(values, strides, fill=0):
    """A flat uint16 memory image of ``values`` uint16 [b, rows, heads, d] at ``strides``, ``fill`` everywhere else."""
    flat = np.full(extent(values.shape, strides), fill, np.uint16)
    view = np.lib.stride_tricks.as_strided(flat, values.shape, tuple(2 * s for s in strides) + (2,))
    view[...] = values
    return flat


def pick(flat, shape, strides):
    return np.lib.stride_tricks.as_strided(flat, shape, tuple(2 * s for s in strides) + (2,)).copy()
