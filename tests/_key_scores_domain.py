"""Float64 reference and error bound of ``daam_key_scores`` (include/daam_analysis.h), shared by ``test_key_scores_cpu.py`` and
``test_gpu_key_scores.py``.

Reference: the windows of a key's planes summed in float64, the bicubic of ``oracle.heatmap_oracle.bicubic_taps`` rows first and
then columns (``_resize64`` of ``tests/test_gpu_rect.py``), the clamp, the dot with every footprint.

Bound, per (key, mask m, token row t):

    |got - exact| <= e_t * sum_p |f_m[p]|  +  c * 2^-24 * sum_p |f_m[p] * K_exact[p]|

* ``e_t = 2^-19 * rowmax_t`` is the accuracy class include/daam_hip.h documents for the f32 bicubic of any finite planes: every
  resized, clamped element is within ``e_t`` of the exact one (the clamp does not grow an error).
* A window range adds ``n_win - 1`` f32 additions per plane element in front of the bicubic.  Each is off by at most ``2^-24`` of its
  partial sum, so an element by at most ``(n_win - 1) 2^-24 rowmax_t`` when ``rowmax_t`` is the largest magnitude among the row's
  partial sums over the windows.  The resize carries that to an output element through 16 tap weights whose magnitudes sum to
  ``(sum_a |wx_a|) (sum_b |wy_b|)``; for Keys' kernel with A = -0.75 one axis gives at most 1.375 (at t = 0.5: 2 x 0.59375 + 2 x
  0.09375), so the product is below 2: ``e_t = (2^-19 + 2 (n_win - 1) 2^-24) rowmax_t``.
* ``c = 2 + chain``: the rounding of the product ``f * K`` (none in the kernel, which uses a fused multiply-add: the bound is kept
  at the looser count), one for ``K`` as an f32 value, and the longest chain of f32 additions on an element's way through the
  kernel's reduction tree, ``reduction_chain`` below: a lane adds its elements ``p = lane, lane + 256, ...`` one after the other,
  six butterfly steps join the 64 lanes of a wave, and two more additions join the four waves as ``(w0 + w1) + (w2 + w3)``.
"""
import numpy as np

from oracle import heatmap_oracle as ho

THREADS = 256


def reduction_chain(cells: int) -> int:
    """Additions on the longest path of one dot product over ``cells`` elements in ``key_scores_kernel``."""
    per_lane = -(-cells // THREADS)            # the lane's own chain (its first product is added to 0)
    butterfly = 6                              # xor 32, 16, 8, 4, 2, 1 inside a wave of 64
    waves = 2                                  # (w0 + w1) + (w2 + w3)
    return per_lane + butterfly + waves


def reduce_like_kernel(products: np.ndarray) -> np.float32:
    """The kernel's tree on f32 ``products`` [cells] (what each fused multiply-add contributes), in f32: the order the bound counts."""
    cells = products.shape[0]
    lanes = np.zeros(THREADS, np.float32)
    for start in range(0, cells, THREADS):
        part = products[start:start + THREADS].astype(np.float32)
        lanes[:part.shape[0]] = lanes[:part.shape[0]] + part
    waves = lanes.reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, np.arange(64) ^ off]
    w = waves[:, 0]
    return np.float32(np.float32(w[0] + w[1]) + np.float32(w[2] + w[3]))


def resize64(planes: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """[..., h, w] -> [..., out_h, out_w] float64: rows first, then columns; a plane of the output's size is a copy."""
    x = planes.astype(np.float64)
    h, w = x.shape[-2:]
    if (h, w) == (out_h, out_w):
        return x
    ix, wx = ho.bicubic_taps(w, out_w, np.float32)
    x = sum(x[..., :, ix[:, a]] * wx[:, a].astype(np.float64) for a in range(4))
    iy, wy = ho.bicubic_taps(h, out_h, np.float32)
    return sum(x[..., iy[:, a], :] * wy[:, a].astype(np.float64)[:, None] for a in range(4))


def clamped64(windows: np.ndarray, out_h: int, out_w: int):
    """``windows`` [n_win, rows, h, w] (any float dtype) -> ``(K [rows, out_h * out_w] float64, rowmax [rows])``."""
    partial = np.cumsum(windows.astype(np.float64), axis=0)
    rowmax = np.abs(partial).max(axis=(0, 2, 3))
    k = np.maximum(resize64(partial[-1], out_h, out_w), 0.0)
    return k.reshape(k.shape[0], -1), rowmax


def reference(windows: np.ndarray, out_h: int, out_w: int, footprint):
    """``(exact [M, rows], bound [M, rows])`` of one key; ``footprint`` [M, out_h, out_w] or ``None`` (one column of ones)."""
    k, rowmax = clamped64(windows, out_h, out_w)
    f = np.ones((1, out_h * out_w)) if footprint is None else footprint.astype(np.float64).reshape(footprint.shape[0], -1)
    return f @ k.T, bound(f, k, rowmax, windows.shape[0])


def row_error(rowmax: np.ndarray, n_win: int) -> np.ndarray:
    return (2.0 ** -19 + 2.0 * (n_win - 1) * 2.0 ** -24) * rowmax


def bound(f: np.ndarray, k: np.ndarray, rowmax: np.ndarray, n_win: int) -> np.ndarray:
    """``f`` [M, cells], ``k`` [rows, cells] (exact, clamped), ``rowmax`` [rows] -> [M, rows]."""
    c = 2 + reduction_chain(f.shape[1])
    return np.abs(f).sum(axis=1)[:, None] * row_error(rowmax, n_win)[None, :] + c * 2.0 ** -24 * (np.abs(f) @ np.abs(k).T)


def worst_ratio(got: np.ndarray, exact: np.ndarray, bnd: np.ndarray, label: str) -> float:
    """max |got - exact| / bound, printed before anyone asserts on it (0 / 0 counts as 0)."""
    err = np.abs(got.astype(np.float64) - exact)
    ratio = np.where(err == 0, 0.0, err / np.where(bnd > 0, bnd, np.finfo(np.float64).tiny))
    worst = float(ratio.max()) if np.isfinite(got).all() else float('inf')
    print(f'key_scores {label}: worst |err| / bound = {worst:.4f}')
    return worst
