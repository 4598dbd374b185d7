"""Shared by ``test_bins_domain_cpu.py`` and ``test_gpu_bins_domain.py``: window planes up to 2^20 apart, the float64 reference of a
window-range finalize (``daam_finalize_bins``), the per-token-row bound it is held to, and a numpy emulation of
``finalize_bin_sum_kernel`` with five mutants.  The planes, the finalize reference, the row metric and the two finalize contracts
are ``_finalize_domain``'s (``fd``); nothing of them is copied here.

Layout.  The library keeps a layer's sums as ONE buffer ``[n_bins][heads, 77, side * side]`` (tokens in front of pixels); key
``(layer, head)`` of window ``b`` starts ``b * heads * 77 * hw + head * 77 * hw`` elements in.  A window-range group
``(set, b0, b1, rows)`` makes one task per selected key: ``n_elem = rows * hw`` elements from the key's start (the crop is contiguous
from token 0), ``n_win = b1 - b0`` windows ``win_stride = heads * 77 * hw`` elements apart, added in window order in f32 into a tight
``[rows, hw]`` f32 scratch plane.  The grouped finalize kernels then run on the scratch planes as f32 sums.

Window planes (``draw_windows``).  Per layer ``[nb, 2 * heads, hw, 77]`` from ``fd.draw_planes``, one seed per window, window ``b``
multiplied by ``2^-(4 * (b % 6))``: windows 0 and 5 lie 2^20 apart, on top of the 2^21 between token rows.  ``signed`` flips random signs
(windows cancel).  ``exact``: the non-negative draw scaled by a power of two to stay below 2^6, rounded to the sums' dtype, then truncated
to a multiple of 2^-10 (no window scale: it would truncate the small windows to zero).  Such numbers stay exact in the sums' dtype, and any
f32 sum of up to 64 of them is below 2^12 on a 2^-10 grid -- 22 bits -- hence exact: the reduction contributes no error, whatever order
it adds in, and a dropped, doubled or mis-strided window cannot hide inside a rounding allowance.  Token rows whose level lies below
2^-10 are zero there (about half of them), and have to come out exactly zero.

Reference.  Float64 sum of the windows as the sums' dtype holds them, then ``fd.reference64`` (bicubic -> clamp -> mean) of the summed
planes of the group's keys, rows ``[0, rows)``.

Bound, per token row ``t`` (``err_t``, ``rowmax_t`` as in ``fd.row_errors``):

    err_t <= REL * rowmax_t + (FLOOR if an MFMA x2 kernel ran) + (n_win - 1) * 2^-24 * max_keys(W_key * S_t,key)

  * The first two terms are ``fd``'s contract of the finalize route that runs on the summed planes.
  * ``S_t,key = max_pixels sum_w |v_w|``.  An in-order f32 sum of n numbers differs from the exact sum by at most
    ``(n - 1) * u * sum |v_w|`` with ``u = 2^-24`` (recursive summation; each add's rounding is at most ``u`` of a partial sum that is at
    most ``sum |v_w|``, and Jeannerod and Rump, 2013, show the bound holds without a second-order term).  fp16 / bf16 / f32 elements widen to
    f32 exactly and an f32 add that underflows is exact, so there is no other source.
  * The bicubic resize is linear: a perturbation of at most ``d`` per source pixel moves an output pixel by at most ``W * d``,
    ``W`` = the product of the two passes' largest absolute tap-weight sums (``max_j sum_a |w[j, a]|`` of ``ho.bicubic_taps`` for the
    side, squared; 1 for a same-size key, which is copied).  ``max(x, 0)`` is 1-Lipschitz and the mean over keys does not exceed the
    largest key's share.
  * A group of ONE window has no reduction term (on the direct path the sums' own dtype decides the route).  ``exact`` planes have none
    either: the test checks that their f32 sum IS the float64 sum.
No number here is measured.

Emulation (``emulate_task``).  What ``finalize_bin_sum_kernel`` does to one task, in numpy f32: a task whose key address and window
stride allow 16-byte accesses (``vec``) goes in pieces of ``V = 16 / sizeof(element)`` elements, the ``n_elem % V`` elements behind the
last whole piece one by one; a task that does not goes one by one altogether.  Rows ``[0, rows)`` only; the scratch starts as zeros.
Mutants: ``skip_last`` (the last window not added), ``short_stride`` (window stride short by one head's planes), ``sum_in_dtype`` (the
running sum rounded to the sums' dtype after every add; for f32 sums that is the kernel itself), ``drop_tail`` (the ``n_elem % V``
elements behind the last whole piece not written) and ``token_stride`` (the key's token block in the SOURCE taken as ``rows * hw``
elements, the scratch's tight layout, instead of ``77 * hw``: head ``h`` is read from ``h * rows * hw``).
"""
import math
from functools import lru_cache

import numpy as np

import _finalize_domain as fd
from oracle import heatmap_oracle as ho

TOKENS = fd.TOKENS
WINDOW_STEP, WINDOW_LEVELS = 4, 6                 # window b sits at 2^-(4 * (b % 6))
U32 = 2.0 ** -24                                  # unit roundoff of f32
EXACT_GRID, EXACT_TOP = 2.0 ** -10, 2.0 ** 6
KINDS = ['levelled', 'signed', 'exact']
DTYPES = fd.DTYPES
ELEM = {'float16': 2, 'bfloat16': 2, 'float32': 4}
VEC = {d: 16 // e for d, e in ELEM.items()}       # elements of a 16-byte piece
TAG = {'float16': 'f16', 'bfloat16': 'bf16', 'float32': 'f32'}
MUTANTS = ['skip_last', 'short_stride', 'sum_in_dtype', 'drop_tail', 'token_stride']
ROWS = [1, 5, 77]

# Cut-piece sets: layers of `sides` with `heads` kept heads each, finalized onto `out_side`; `offset`: elements between a 16-byte boundary
# and the start of every layer's buffer.  `reaches`: the branches of the reduction the set is there for, per element size, at every row
# count of ROWS -- asserted from addresses and sizes (`branches`), not taken on trust.
#   s6_12_24      16 bit: 3 * 77 * 36 * 2 bytes per window is 8 mod 16 -> side 6 goes element by element, sides 12 / 24 in whole pieces.
#                 f32:    every window stride and key address is a multiple of 16 and 36 % 4 == 0: whole pieces only.
#   s8_32         the aligned control: whole pieces only.
#   s8_32_off1    the same planes one element off a 16-byte boundary: element by element.
#   s6_12_h2      16 bit, two heads: head 0 of side 6 is aligned and rows * 36 is 4 mod 8 at odd rows: pieces + a cut piece; head 1 starts
#                 8 bytes off: element by element.
#   s3_6_h4       f32 needs an odd side and a multiple of four heads for an aligned key with a cut piece (77 * hw * 4 * heads % 16 == 0 and
#                 rows * hw % 4 != 0): side 3, four heads, head 0.  Four heads of 9 and 36 pixels: smaller than any other set.
CUT_SETS = {
    's6_12_24': dict(sides=(6, 12, 24), heads=3, out_side=48, offset=0,
                     reaches={2: {'elementwise', 'pieces'}, 4: {'pieces'}}),
    's8_32': dict(sides=(8, 32), heads=1, out_side=64, offset=0, reaches={2: {'pieces'}, 4: {'pieces'}}),
    's8_32_off1': dict(sides=(8, 32), heads=1, out_side=64, offset=1, reaches={2: {'elementwise'}, 4: {'elementwise'}}),
    's6_12_h2': dict(sides=(6, 12), heads=2, out_side=48, offset=0,
                     reaches={2: {'pieces+tail', 'elementwise', 'pieces'}, 4: {'pieces'}}),
    's3_6_h4': dict(sides=(3, 6), heads=4, out_side=48, offset=0,
                    reaches={2: {'pieces+tail', 'elementwise'}, 4: {'pieces+tail', 'elementwise', 'pieces'}}),
}
CUT_NB = 3                                        # windows of a cut-piece context; every group takes [0, 3)
COUNT_NB, COUNT_SIDES, COUNT_HEADS = 50, (32, 64), 1
COUNT_RANGES = [(0, 2), (10, 17), (0, 50)]        # n_win 2, 7, 50


def window_scale(b):
    return 2.0 ** -(WINDOW_STEP * (b % WINDOW_LEVELS))


def draw_windows(sides, kind, nb, heads, seed=0):
    """The windows of every layer as float32, not yet rounded: ``[nb, 2 * heads, hw, 77]`` each (unconditional half zero)."""
    variant = 'signed' if kind == 'signed' else 'nonneg'
    per_window = [fd.draw_planes(sides, variant, heads, seed=1000 * seed + 17 + b) for b in range(nb)]
    out = []
    for layer in range(len(sides)):
        w = np.stack([per_window[b][layer] for b in range(nb)])
        if kind == 'exact':
            w *= np.float32(2.0 ** fd.scale_exp([w], 0, EXACT_TOP * (1 - 2.0 ** -9)))
        else:
            w *= np.float32([window_scale(b) for b in range(nb)]).reshape(nb, 1, 1, 1)
        out.append(w)
    return out


def round_windows(windows, kind, dtype):
    """To the sums' dtype (``fd.round_to``); ``exact``: then truncated to multiples of 2^-10, which the dtype still holds."""
    got = []
    for w in windows:
        r = fd.round_to(w, dtype)
        if kind == 'exact':
            r = (np.trunc(r.astype(np.float64) / EXACT_GRID) * EXACT_GRID).astype(r.dtype)
            assert np.array_equal(fd.round_to(r.astype(np.float32), dtype), r) and float(np.abs(r.astype(np.float64)).max()) < EXACT_TOP
        got.append(r)
    return got


def native(windows):
    """``[nb, 2 * heads, hw, 77]`` per layer -> the kept half as the library holds it, ``[nb, heads, 77, hw]`` (``ho.unravel`` per window)."""
    return [np.stack([ho.unravel(w[b]).reshape(w.shape[1] - w.shape[1] // 2, TOKENS, -1) for b in range(w.shape[0])]) for w in windows]


@lru_cache(maxsize=2)
def _drawn(sides, kind, nb, heads, seed):
    return draw_windows(sides, kind, nb, heads, seed)


def native_windows(sides, kind, nb, heads, dtype, seed=0):
    """``native(round_windows(draw_windows(...)))``: per layer ``[nb, heads, 77, hw]`` in the sums' dtype (bf16 numbers as float32)."""
    return native(round_windows(_drawn(tuple(sides), kind, nb, heads, seed), kind, dtype))


def key_table(sides, heads):
    """Key i of the context -> (layer, head): layers in order, heads inside (the library's key order)."""
    return [(layer, h) for layer in range(len(sides)) for h in range(heads)]


# ---- reference and bound ---------------------------------------------------------------------------------------------------------
def tap_gain(side, out_side):
    """W of the bound: 1 for a same-size key (copied), else the squared largest absolute tap-weight sum of the side's bicubic taps."""
    if side == out_side:
        return 1.0
    _, w = ho.bicubic_taps(side, out_side, np.float64)
    return float(np.abs(w).sum(1).max()) ** 2


def _summed(planes, keys, b0, b1, rows):
    """Per layer with a selected key: ``(layer, float64 window sum [h', rows, hw], sum of magnitudes)`` of the group's keys."""
    out = []
    for layer in sorted({l for l, _ in keys}):
        hs = [h for l, h in keys if l == layer]
        v = planes[layer][b0:b1, hs, :rows].astype(np.float64)
        out.append((layer, v.sum(0), np.abs(v).sum(0)))
    return out


def reference(planes, sides, out_side, keys, b0, b1, rows):
    """``(want64 [rows, out, out], reduction allowance [rows], is the f32 window sum exact)`` of one group over ``keys`` (a list of
    ``(layer, head)``): the float64 reference and ``(n_win - 1) * 2^-24 * max_keys(W_key * S_t,key)``."""
    parts = _summed(planes, keys, b0, b1, rows)
    as_probs = [np.concatenate([np.zeros_like(s), s]).transpose(0, 2, 1) for _, s, _ in parts]       # [2 * h', hw, rows]
    want = fd.reference64(as_probs, [sides[l] for l, _, _ in parts], out_side)
    gain = np.max([tap_gain(sides[l], out_side) * mag.max((0, 2)) for l, _, mag in parts], axis=0)
    exact = True
    for l, s, _ in parts:
        hs = [h for ll, h in keys if ll == l]
        acc = np.zeros(s.shape, np.float32)
        for b in range(b0, b1):
            acc = acc + planes[l][b, hs, :rows].astype(np.float32)
        exact = exact and np.array_equal(acc.astype(np.float64), s)
    return want, (b1 - b0 - 1) * U32 * gain, exact


def bound(rowmax, allowance, mfma):
    return fd.contract_bound(rowmax, mfma) + allowance


def check(got, want, allowance, mfma, what):
    """The bound, row by row; returns ``(worst err_t / bound_t, worst err_t / rowmax_t)``.  A row whose bound is zero must be exact."""
    assert np.isfinite(np.asarray(got)).all(), f'{what}: non-finite output'
    err, rowmax = fd.row_errors(got, want)
    lim = bound(rowmax, allowance, mfma)
    bad = np.nonzero(err > lim)[0]
    assert bad.size == 0, (f'{what}: {bad.size} token rows outside the bound; worst rows ' +
                           ', '.join(f't={t} err {err[t]:.3e} (rowmax {rowmax[t]:.3e}, bound {lim[t]:.3e})'
                                     for t in bad[np.argsort(-(err[bad] / np.maximum(lim[bad], 1e-300)))][:4]))
    live = lim > 0
    return (float((err[live] / lim[live]).max()) if live.any() else 0.0,
            float((err[rowmax > 0] / rowmax[rowmax > 0]).max()) if (rowmax > 0).any() else 0.0)


def misses(got, want, allowance, mfma):
    """Does ``got`` break the bound on some token row?  (What a mutant is expected to do.)"""
    err, rowmax = fd.row_errors(got, want)
    return bool((err > bound(rowmax, allowance, mfma)).any()) or not np.isfinite(np.asarray(got)).all()


def report(what, names, branches, ratio, rel):
    print(f'\nBINDOMAIN {what} | {"+".join(sorted(names))} | reduction: {"+".join(sorted(branches)) or "none"} | '
          f'err_t/bound_t <= {ratio:.3f} | err_t/rowmax_t <= 2^{math.log2(max(rel, 1e-300)):.2f}')


# ---- the reduction's tasks -------------------------------------------------------------------------------------------------------
def plan_task(side, heads, dtype, layer_addr, head, b0, b1, rows):
    """One task as ``daam_finalize_bins`` builds it for key ``head`` of a layer whose buffer starts at byte address ``layer_addr``."""
    hw, elem = side * side, ELEM[dtype]
    layer_bytes = heads * TOKENS * hw * elem
    src = layer_addr + (b0 * heads + head) * TOKENS * hw * elem
    return dict(src_off=(b0 * heads + head) * TOKENS * hw, win_stride=heads * TOKENS * hw, n_elem=rows * hw, n_win=b1 - b0, hw=hw,
                head=head, b0=b0, heads=heads, rows=rows, vec=(src | layer_bytes) % 16 == 0)


def branch_of(task, dtype):
    """Which text of the kernel a task runs: ``pieces`` (16-byte pieces only), ``pieces+tail`` (and a cut last piece, element by element)
    or ``elementwise`` (no 16-byte access at all)."""
    if not task['vec']:
        return 'elementwise'
    return 'pieces+tail' if task['n_elem'] % VEC[dtype] else 'pieces'


def branches(sides, heads, dtype, layer_addrs, keys, b0, b1, rows):
    return {branch_of(plan_task(sides[l], heads, dtype, layer_addrs[l], h, b0, b1, rows), dtype) for l, h in keys}


def _add(acc, v, carry):
    if carry == 'float16':
        return (acc.astype(np.float32) + v.astype(np.float32)).astype(np.float16)
    s = acc.astype(np.float32) + v.astype(np.float32)
    return ho.round_bf16(s) if carry == 'bfloat16' else s


def emulate_task(buf, task, dtype, mutant=None):
    """The f32 scratch plane ``[rows * hw]`` of one task from the layer's flat buffer ``buf`` (all windows, the sums' dtype)."""
    n, hw, v = task['n_elem'], task['hw'], VEC[dtype]
    stride = task['win_stride'] - (TOKENS * hw if mutant == 'short_stride' else 0)
    off = task['src_off']
    if mutant == 'token_stride':
        off = task['b0'] * task['win_stride'] + task['head'] * task['rows'] * hw
    n_win = task['n_win'] - (mutant == 'skip_last')
    carry = dtype if mutant == 'sum_in_dtype' else 'float32'
    whole = n // v * v
    out = np.zeros(n, np.float32)
    # (whole pieces and one-by-one elements add the same numbers in the same order: what differs is which elements a fault can drop)
    for lo, hi in [(0, whole), (whole, n)]:
        if hi <= lo or (mutant == 'drop_tail' and lo == whole):
            continue
        acc = np.zeros(hi - lo, np.float16 if carry == 'float16' else np.float32)
        for w in range(n_win):
            acc = _add(acc, buf[off + w * stride + lo:off + w * stride + hi], carry)
        out[lo:hi] = acc.astype(np.float32)
    return out


def emulate_group(planes, sides, heads, dtype, out_side, keys, b0, b1, rows, mutant=None, offset=0):
    """The reduction emulated for every key of a group, then the float64 finalize of the scratch planes: ``[rows, out, out]``."""
    by_layer = {}
    for l, h in keys:
        task = plan_task(sides[l], heads, dtype, 4096 + offset * ELEM[dtype], h, b0, b1, rows)
        plane = emulate_task(planes[l].reshape(-1), task, dtype, mutant)
        by_layer.setdefault(l, []).append(plane.reshape(rows, -1).astype(np.float64))
    layers = sorted(by_layer)
    as_probs = [np.concatenate([np.zeros_like(np.stack(by_layer[l])), np.stack(by_layer[l])]).transpose(0, 2, 1) for l in layers]
    return fd.reference64(as_probs, [sides[l] for l in layers], out_side)
