"""Shared by ``test_rect_domain_cpu.py`` and ``test_gpu_rect_domain.py`` (and, for the reference, ``test_gpu_rect.py``): the
rectangular finalize (``finalize_rect_kernel`` / ``finalize_rect_grouped_kernel``, daam_amd/csrc/daam_finalize_rect.hip) held to
float64 on key walks of more than one key per workgroup.

Reference.  ``resize64`` / ``global64``: float64 numpy, ``oracle.heatmap_oracle.bicubic_taps`` (torch's f32 coefficients) along the rows
and then down the columns, clamp at 0, mean over the keys.

Levelled rectangular planes.  The recipe of ``_finalize_domain.draw_planes`` on ``(h, w)`` shapes, in the layout the device holds
(``[heads, 77, h, w]`` per layer): ``exp(standard_normal)``, token ``t`` times ``2^-(3 * (t % 8))``; ``signed`` flips random signs (the clamp
matters).  Scaling by ``2^k``, rounding to the sums' dtype, the per-token-row error metric and the worst-ratio report are
``_finalize_domain``'s own functions, unchanged.

Contract, per token row ``t`` with ``err_t = max_pixels |got[t] - want64[t]|`` and ``rowmax_t = max_pixels |want64[t]|``, for a mean over
``N`` keys:

    err_t <= (2^-19 + max(0, N - 6) * 2^-24) * rowmax_t

``2^-19 * rowmax_t`` is the exact-f32 contract ``_finalize_domain`` documents for selections of at most 6 keys per mean (the f32
four-tap sums of both passes and at most 6 f32 adds over the keys come to under 2^-20 of the row's maximum).  Every further key is
one further f32 addition: the tile (or the atomic) takes ``partial + term``, rounded, off by at most half an ulp = ``2^-24`` of that
partial sum.  The terms are clamped non-negative, so a partial sum never exceeds the full sum ``N * mean``; times ``1 / N`` the extra
error per key is at most ``2^-24 * mean <= 2^-24 * rowmax_t``.  No other tolerance exists here.

Host plan.  ``plan_chunks(max_n, sum_rows)`` restates ``fin_rect()`` (daam_finalize_api.hip): ``n_chunks = max(1, min(max_n, (1024 +
sum_rows / 2) / sum_rows))`` in integer arithmetic; workgroup ``(t, c)`` walks keys ``c, c + n_chunks, ...`` of its group (``walks``).

Emulation.  ``emulate``: the kernel's own order in float32 numpy -- per workgroup an LDS plane buffer, the row pass, then the column
pass with the f32 tap weights of ``ho.bicubic_taps`` (a key of the output's size is copy + clamp), ``tile += max(v, 0)`` key after key
in walk order, and the chunks' ``tile * inv_n`` added in chunk order (on the device the atomics arrive in any order).  ``mutant=`` names
a deliberate defect (``MUTANTS``) the contract has to catch.

Cases (``CASES``; all 77 token rows unless ``rows`` says otherwise; key j of a context is head ``j`` counted through the layers in
order):

  multi_walk_single  (12, 20) from (6, 10), (12, 20), (3, 5) x 8 heads = 24 keys, one map: 13 chunks, workgroups 0 .. 10 walk keys
                     c and c + 13.  In this layer order chunks 0 .. 2 take a x2 key and then a same-size (copy) key, chunks 3 .. 7 a x2
                     and then a x4 key (a 15-element plane in the tile behind a 60-element one), chunks 8 .. 10 a copy key and then
                     a x4 key: copy after table and table after copy both happen.
  one_chunk_groups   the same 24 key shapes in 12 groups of 2 over 77 rows each: one chunk, every workgroup walks both keys of its
                     group.  The layers are split ((3, 5) x 4, (12, 20) x 4, (6, 10) x 8, (12, 20) x 4, (3, 5) x 4) so that the groups pair
                     x4 -> copy, x4 -> x2 (small plane, then large), copy -> x2, copy -> x4, x2 -> x4 (large, then small), x2 -> copy.
  unequal_groups     6 keys, group 0 = one (copy) key, group 1 = five, rows [77, 9]: 5 chunks, four of group 0's hold no key.
  pieces_mix_16x24   (16, 24) from (8, 12), (16, 24), (4, 6) x 8: 96 / 384 / 24 elements, 16-byte pieces in every dtype; the walk of
                     multi_walk_single.
  pieces_mix_14x6    (14, 6) from (7, 3), (14, 6) x 8: 21 / 84 elements, 16-bit token rows that are no whole number of 16-byte pieces
                     (element by element), f32 rows of 84 in pieces and of 21 element by element; chunks 0 .. 2 walk a table key
                     and then a copy key.
  mixed_axes         (12, 20) from (12, 10) (rows are a copy), (6, 20) (columns are a copy), (24, 40) (x0.5), (12, 30) (shrinks on one axis
                     only) x 2 heads: 8 keys, 8 chunks."""
import math

import numpy as np

import _finalize_domain as fd
from oracle import heatmap_oracle as ho

TOKENS = fd.TOKENS
EXTRA_PER_KEY = 2.0 ** -24           # one further f32 addition per key beyond 6 (module docstring)
MUTANTS = ('swap_tables', 'no_clamp', 'clamp_after_mean', 'inv_max_n', 'overwrite', 'first_w', 'drop_last_column')
TAG = {'float16': 'f16', 'bfloat16': 'bf16', 'float32': 'f32'}


# ---- the float64 reference -------------------------------------------------------------------------------------------------------
def resize64(planes, out_h, out_w):
    """[..., h, w] -> [..., out_h, out_w] float64: rows first, then columns (torch's order); an axis of the output's size is a copy."""
    x = planes.astype(np.float64)
    h, w = x.shape[-2:]
    if w != out_w:
        ix, wx = ho.bicubic_taps(w, out_w, np.float32)
        x = sum(x[..., :, ix[:, a]] * wx[:, a].astype(np.float64) for a in range(4))
    if h != out_h:
        iy, wy = ho.bicubic_taps(h, out_h, np.float32)
        x = sum(x[..., iy[:, a], :] * wy[:, a].astype(np.float64)[:, None] for a in range(4))
    return x


def global64(key_planes, out_h, out_w):
    """mean over keys of clamp(resize(plane), 0); ``key_planes``: list of [77, h, w]."""
    return sum(np.maximum(resize64(p, out_h, out_w), 0) for p in key_planes) / len(key_planes)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def _case(out_hw, layers, key_group=None, rows=None):
    return dict(out_hw=out_hw, layers=layers, key_group=key_group, rows=rows)


def _pair_groups():
    """one_chunk_groups: keys 0-3 x4, 4-7 copy, 8-15 x2, 16-19 copy, 20-23 x4 (module docstring)."""
    pairs = [(0, 4), (1, 5), (2, 8), (3, 9), (6, 10), (7, 11), (16, 20), (17, 21), (12, 22), (13, 23), (14, 18), (15, 19)]
    kg = [-1] * 24
    for g, (a, b) in enumerate(pairs):
        kg[a] = kg[b] = g
    assert sorted(kg) == sorted(list(range(12)) * 2)
    return kg


CASES = {
    'multi_walk_single': _case((12, 20), [((6, 10), 8), ((12, 20), 8), ((3, 5), 8)]),
    'one_chunk_groups': _case((12, 20), [((3, 5), 4), ((12, 20), 4), ((6, 10), 8), ((12, 20), 4), ((3, 5), 4)], _pair_groups(), [TOKENS] * 12),
    'unequal_groups': _case((12, 20), [((6, 10), 2), ((12, 20), 2), ((3, 5), 2)], [1, 1, 0, 1, 1, 1], [TOKENS, 9]),
    'pieces_mix_16x24': _case((16, 24), [((8, 12), 8), ((16, 24), 8), ((4, 6), 8)]),
    'pieces_mix_14x6': _case((14, 6), [((7, 3), 8), ((14, 6), 8)]),
    'mixed_axes': _case((12, 20), [((12, 10), 2), ((6, 20), 2), ((24, 40), 2), ((12, 30), 2)]),
}
MAGNITUDE_CASES = ('multi_walk_single', 'mixed_axes')        # every k of fd.K_EXACT (+ 40), both variants; the others k = 0, signed
KEY_MASK = [0 if j % 5 in (1, 3) else 1 for j in range(24)]  # multi_walk_single with 14 keys left: chunk 0 walks keys 0 (x2) and 22 (x4)


def key_shapes(case):
    """(h, w) of every key of the context, in key order."""
    return [hw for hw, heads in CASES[case]['layers'] for _ in range(heads)]


def groups_of(case, key_mask=None, n_rows=None):
    """``[(key indices, rows)]``: the maps one call makes -- one for a single finalize (``key_mask`` / ``n_rows`` as daam_finalize takes
    them), one per group for a grouped case."""
    c = CASES[case]
    n = len(key_shapes(case))
    if c['key_group'] is None:
        return [([j for j in range(n) if key_mask is None or key_mask[j]], n_rows or TOKENS)]
    assert key_mask is None and n_rows is None
    return [([j for j in range(n) if c['key_group'][j] == g], r) for g, r in enumerate(c['rows'])]


def plan_chunks(max_n, sum_rows):
    """``n_chunks`` of ``fin_rect()`` for groups of at most ``max_n`` keys over ``sum_rows`` token rows in all."""
    return max(1, min(max_n, (1024 + sum_rows // 2) // sum_rows))


def plan_of(groups):
    """``(n_chunks, grid)`` of the launch that serves ``groups``: grid = largest row count x chunks x groups."""
    n_chunks = plan_chunks(max(len(keys) for keys, _ in groups), sum(rows for _, rows in groups))
    return n_chunks, max(rows for _, rows in groups) * n_chunks * len(groups)


def walks(n_keys, n_chunks):
    """Positions (in the group's own key list) workgroup ``c`` walks, for every chunk."""
    return [list(range(c, n_keys, n_chunks)) for c in range(n_chunks)]


def keys_per_workgroup(groups):
    """The longest walk of the launch that serves ``groups``."""
    n_chunks, _ = plan_of(groups)
    return max(math.ceil(len(keys) / n_chunks) for keys, _ in groups)


def key_kind(shape, out_hw, dtype):
    """``('copy' | 'table', 'pieces' | 'elements')`` of a key: how ``finalize_rect_body`` reads and applies it.  A token row is a whole
    number of 16-byte pieces when ``h * w`` is a multiple of 8 (16-bit) resp. 4 (f32) elements; every token row then starts on a 16-byte
    boundary as well (the buffers do)."""
    n = shape[0] * shape[1]
    per = 4 if dtype == 'float32' else 8
    return 'copy' if tuple(shape) == tuple(out_hw) else 'table', 'pieces' if n % per == 0 else 'elements'


# ---- levelled rectangular planes -------------------------------------------------------------------------------------------------
def draw_planes(case, variant, seed=0):
    """The k = 0 planes of every layer as float32 (not yet rounded to the sums' dtype): ``[heads, 77, h, w]`` each."""
    layers = CASES[case]['layers']
    rng = np.random.default_rng([seed, list(CASES).index(case), len(layers), fd.VARIANTS.index(variant)])
    lev = fd.token_levels().astype(np.float32)[None, :, None, None]
    out = []
    for (h, w), heads in layers:
        x = np.exp(rng.standard_normal((heads, TOKENS, h, w))).astype(np.float32)
        if variant == 'signed':
            x *= rng.choice(np.float32([-1.0, 1.0]), size=x.shape)
        out.append(x * lev)
    return out


def exponents(dtype):
    return fd.K_EXACT + ([40] if dtype != 'float16' else [])


def planes_at(case, variant, k, dtype):
    """``(k really applied, planes rounded to dtype)``: fp16 sums stay inside ``fd.DOMAIN_MAX`` (``fd.scale_exp``)."""
    base = draw_planes(case, variant)
    k = fd.scale_exp(base, k, fd.DOMAIN_MAX if dtype == 'float16' else None)
    planes, _ = fd.scaled_planes(base, k, dtype)
    return k, planes


def key_planes(planes):
    """Per-layer ``[heads, 77, h, w]`` -> the context's keys ``[77, h, w]`` as float32 values, in key order."""
    return [np.asarray(p[h], np.float32) for p in planes for h in range(p.shape[0])]


def reference(keys, out_hw, groups):
    """float64 maps ``[rows, out_h, out_w]`` of every group."""
    return [global64([keys[j] for j in idx], *out_hw)[:rows] for idx, rows in groups]


# ---- contract --------------------------------------------------------------------------------------------------------------------
def rel_bound(n_keys):
    return fd.REL + max(0, n_keys - 6) * EXTRA_PER_KEY


def assert_contract(got, want64, n_keys, what, times=1.0):
    """``err_t <= times * rel_bound(n_keys) * rowmax_t`` on every token row; returns the worst ``err_t / rowmax_t``."""
    if n_keys <= 6 and times == 1.0:
        return fd.assert_contract(got, want64, False, what)[0]
    assert np.isfinite(np.asarray(got)).all(), f'{what}: non-finite output'
    err, rowmax = fd.row_errors(got, want64)
    bound = times * rel_bound(n_keys) * rowmax
    bad = np.nonzero(err > bound)[0]
    rel, _ = fd.worst(err, rowmax)
    assert bad.size == 0, (f'{what}: {bad.size} token rows outside the contract for {n_keys} keys; worst rows ' +
                           ', '.join(f't={t} err {err[t]:.3e} (rowmax {rowmax[t]:.3e}, bound {bound[t]:.3e})'
                                     for t in bad[np.argsort(-(err[bad] / np.maximum(bound[bad], 1e-300)))][:4]))
    return rel


def log2(x):
    return math.log2(max(x, 1e-300))


# ---- the kernel's own order, float32 ---------------------------------------------------------------------------------------------
def _passes32(buf, h, w, stride, out_hw, mutant):
    """Row pass, then column pass on the LDS plane ``buf`` [rows, cap] read through ``stride``; every product and add rounded to f32."""
    oh, ow = out_hw
    ix, wx = ho.bicubic_taps(h if mutant == 'swap_tables' else w, ow, np.float32)
    iy, wy = ho.bicubic_taps(h, oh, np.float32)
    at = (np.arange(h) * stride)[:, None, None] + ix[None, :, :]                  # [h, ow, 4]
    tmp = buf[:, at[..., 0]] * wx[:, 0]
    for a in range(1, 4):
        tmp = tmp + buf[:, at[..., a]] * wx[:, a]
    v = tmp[:, iy[:, 0], :] * wy[:, 0][:, None]
    for a in range(1, 4):
        v = v + tmp[:, iy[:, a], :] * wy[:, a][:, None]
    assert tmp.dtype == np.float32 and v.dtype == np.float32
    return v


def emulate(keys, out_hw, n_chunks, inv_n=None, mutant=None):
    """One map of ``keys`` (list of [rows, h, w] float32 values) as ``finalize_rect_body`` forms it with ``n_chunks`` workgroups per
    token row; ``inv_n``: the factor at the flush (default: this map's own ``1 / len(keys)``)."""
    assert mutant is None or mutant in MUTANTS, mutant
    oh, ow = out_hw
    rows = keys[0].shape[0]
    inv = np.float32(1.0) / np.float32(len(keys)) if inv_n is None else np.float32(inv_n)
    cap = max([k.shape[1] * k.shape[2] for k in keys if k.shape[1:] != (oh, ow)] + [4])
    out = np.zeros((rows, oh, ow), np.float32)
    for walk in walks(len(keys), n_chunks):
        tile = np.zeros((rows, oh, ow), np.float32)
        buf = np.zeros((rows, cap), np.float32)                                    # the LDS plane region; stale data stays
        for step, j in enumerate(walk):
            p = np.asarray(keys[j], np.float32)
            h, w = p.shape[1:]
            if (h, w) == (oh, ow):
                v = p
            else:
                buf[:, :h * w] = p.reshape(rows, -1)
                stride = keys[walk[0]].shape[2] if mutant == 'first_w' and step else w
                v = _passes32(buf, h, w, stride, out_hw, mutant)
            term = v if mutant in ('no_clamp', 'clamp_after_mean') else np.maximum(v, np.float32(0))
            if mutant == 'drop_last_column':
                term = term.copy()
                term[..., ow - 1] = 0
            tile = term if mutant == 'overwrite' and step else tile + term
        out = out + tile * inv
    if mutant == 'clamp_after_mean':
        out = np.maximum(out, np.float32(0))
    assert out.dtype == np.float32
    return out


def emulate_groups(keys, out_hw, groups, mutant=None):
    """Every group's map with the chunk count the host would choose for the launch."""
    n_chunks, _ = plan_of(groups)
    max_n = max(len(idx) for idx, _ in groups)
    return [emulate([keys[j][:rows] for j in idx], out_hw, n_chunks, 1.0 / max_n if mutant == 'inv_max_n' else None,
                    None if mutant == 'inv_max_n' else mutant) for idx, rows in groups]
