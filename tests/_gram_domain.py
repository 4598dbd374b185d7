"""Float64 reference and error bound of ``daam_token_gram`` (include/daam_analysis.h), shared by ``test_token_gram_cpu.py`` and
``test_gpu_token_gram.py``.

Reference: the windows of a key's planes summed in float64, then ``A @ A.T`` in float64.

Bound, per (key, i, j), with ``a`` the exact window sums [rows, hw]:

    |got - exact| <= (c * 2^-23 + r * 2^-24) * sum_p (|a_i| + d_i)(|a_j| + d_j)  +  sum_p (d_i |a_j| + |a_i| d_j + d_i d_j)

* ``c`` = ``chain(hw, wide)``: the longest chain of f32 additions AS BUILT (daam_token_gram.hip).  A key's pixels are cut into chunks
  of 1024; four waves share a chunk.
    - 16-bit path (fp16 / bf16 planes, one window): the chunk is staged in sub-tiles of 128 pixels = 8 k-steps of
      ``v_mfma_f32_32x32x16``; a wave takes 2 k-steps of every sub-tile, one accumulator.  An MFMA adds 16 products and the
      accumulator: 16 additions.  So ``2 * 16`` per sub-tile, ``ceil(min(hw, 1024) / 128)`` sub-tiles (a partly filled sub-tile is
      padded with zeros and still runs all of its k-steps).
    - f32 path (f32 planes, or more than one window): sub-tiles of 64 pixels = 32 k-steps of ``v_mfma_f32_32x32x2_f32``, 8 per
      wave, 2 additions each (a k-ordered fused multiply-add chain): ``16`` per sub-tile, ``ceil(min(hw, 1024) / 64)`` sub-tiles.
    - the four waves are joined as ``(w0 + w1) + (w2 + w3)``: 2.
    - the chunks are added in chunk order: ``ceil(hw / 1024) - 1``.
  Every addition is allowed ``2^-23`` rather than ``2^-24`` of the magnitudes it has summed so far, the rounding of an MFMA's internal
  additions not being documented.  The 16-bit products are exact in f32 (11 x 11 or 8 x 8 significant bits; fp16 subnormals are
  2^-24 steps and their products normal f32 numbers), so the chain is that path's only error.
* ``r`` = 1 on the f32 path: one rounding per product (the fused chain has none; the bound keeps the looser count).
* ``d`` = ``2 (n_win - 1) 2^-24 * max |partial sum|`` per element: the f32 additions of the windows in front of the products.  The
  kernel multiplies ``a + delta`` with ``|delta| <= d``, which the second sum carries through the product and the first through the
  chain.
"""
import numpy as np

CHUNK = 1024
SUB16, SUB32 = 128, 64


def n_chunks(hw: int) -> int:
    return -(-hw // CHUNK)


def chain(hw: int, wide: bool) -> int:
    """Additions on the longest path from a product to ``gram[k][i][j]`` for a key of ``hw`` pixels."""
    px = min(hw, CHUNK)
    per_wave = -(-px // SUB32) * 8 * 2 if wide else -(-px // SUB16) * 2 * 16
    return per_wave + 2 + (n_chunks(hw) - 1)


def reference(windows: np.ndarray, wide: bool):
    """``windows`` [n_win, rows, hw] (any float dtype; the values the device holds) -> ``(exact [rows, rows], bound [rows, rows])``
    in float64.  ``wide``: the f32 path (f32 planes or ``n_win > 1``)."""
    n_win, _, hw = windows.shape
    assert wide or n_win == 1
    partial = np.cumsum(windows.astype(np.float64), axis=0)
    a = partial[-1]
    mag = np.abs(a)
    d = 2.0 * (n_win - 1) * 2.0 ** -24 * np.abs(partial).max(axis=0)
    c = chain(hw, wide)
    grown = mag + d
    bound = (c * 2.0 ** -23 + (2.0 ** -24 if wide else 0.0)) * (grown @ grown.T) + (d @ mag.T + mag @ d.T + d @ d.T)
    return a @ a.T, bound


def cosine(gram: np.ndarray, eps: float = 1e-12) -> np.ndarray:
    diag = np.diagonal(gram, axis1=-2, axis2=-1)
    return gram / np.sqrt(diag[..., :, None] * diag[..., None, :] + eps)


def word_cosine(planes: np.ndarray, rows_a, rows_b, eps: float = 1e-12) -> float:
    """The cosine of two explicitly merged word maps (the mean of each word's token rows) of ``planes`` [rows, hw], in float64."""
    x = planes.astype(np.float64)
    a, b = x[list(rows_a)].mean(axis=0), x[list(rows_b)].mean(axis=0)
    return float(a @ b / np.sqrt((a @ a) * (b @ b) + eps))


def worst_ratio(got: np.ndarray, exact: np.ndarray, bnd: np.ndarray, label: str) -> float:
    """max |got - exact| / bound, printed before anyone asserts on it (0 / 0 counts as 0)."""
    err = np.abs(got.astype(np.float64) - exact)
    ratio = np.where(err == 0, 0.0, err / np.where(bnd > 0, bnd, np.finfo(np.float64).tiny))
    worst = float(ratio.max()) if np.isfinite(got).all() else float('inf')
    print(f'token_gram {label}: worst |err| / bound = {worst:.4f}')
    return worst
