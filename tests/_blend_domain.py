"""Float64 reference and error bound of ``daam_key_blend`` (include/daam_analysis.h), shared by ``test_key_blend_cpu.py`` and
``test_gpu_key_blend.py``.

Reference: per key the clamped, resized map ``K_k`` of ``tests/_key_scores_domain.py`` (``clamped64``: the windows summed in
float64, the bicubic of the oracle rows first and then columns, the clamp), then ``exact[g] = sum_k w64[g][k] * K_k``.

Bound, per set g, token row t and output element p:

    |got - exact| <= sum_k |w_gk| * e_k,t  +  c * 2^-24 * sum_k |w_gk * K_k[t][p]|

* ``e_k,t = row_error`` of key k's row t: every resized, clamped element of the kernel is within it of the exact one (the class
  the key scores are held to, the windows' additions included).
* ``c = chain(n_keys)`` counts the roundings between ``K`` and the output on the kernel's real chain: 1 for ``K`` as an f32 value,
  1 for the product ``w * K`` (contraction is off: the product is rounded on its own), one per addition inside a chunk -- a
  workgroup adds the keys of its chunk of ``CHUNK`` in key order, so at most ``min(n_keys, CHUNK)``, the first of them onto 0 --
  and, when the call has more than one chunk, one per chunk the join kernel adds (again the first onto 0).  A key of zero weight
  is skipped, which only shortens the chain.
"""
import numpy as np

from _key_scores_domain import clamped64, row_error, worst_ratio  # noqa: F401 -- worst_ratio is re-exported to the tests

CHUNK = 32                                     # kBlendChunk: key k belongs to chunk k // CHUNK, whatever n_keys is
MAX_SETS = 8


def n_chunks(n_keys: int) -> int:
    return -(-n_keys // CHUNK)


def chain(n_keys: int) -> int:
    """Roundings on the longest path from a key's exact ``K`` to an output element, as a function of ``n_keys`` alone."""
    chunks = n_chunks(n_keys)
    return 2 + min(n_keys, CHUNK) + (chunks if chunks > 1 else 0)


def key_maps(windows, out_h: int, out_w: int):
    """``windows``: per key an array [n_win, rows, h, w].  -> ``(K [n_keys, rows, cells] float64, e [n_keys, rows])``."""
    maps, errs = [], []
    for win in windows:
        k, rowmax = clamped64(win, out_h, out_w)
        maps.append(k)
        errs.append(row_error(rowmax, win.shape[0]))
    return np.stack(maps), np.stack(errs)


def reference(windows, weights: np.ndarray, out_h: int, out_w: int):
    """``(exact, bound)``, each [n_sets, rows, cells] float64; ``weights`` [n_sets, n_keys] (the f32 values the kernel reads)."""
    k, e = key_maps(windows, out_h, out_w)
    return blend64(k, e, weights)


def blend64(k: np.ndarray, e: np.ndarray, weights: np.ndarray):
    w = weights.astype(np.float64)
    exact = np.einsum('gk,ktp->gtp', w, k)
    c = chain(k.shape[0])
    bound = np.einsum('gk,kt->gt', np.abs(w), e)[:, :, None] + c * 2.0 ** -24 * np.einsum('gk,ktp->gtp', np.abs(w), np.abs(k))
    return exact, bound


def blend_like_kernel(k32: np.ndarray, w32: np.ndarray) -> np.ndarray:
    """The kernel's add order in f32 on f32 maps ``k32`` [n_keys, ...] and one set's weights ``w32`` [n_keys]: inside a chunk the
    keys of non-zero weight in key order onto 0, then -- more than one chunk -- the chunks that hold such a key in chunk order
    onto 0.  The order the bound counts."""
    n_keys = k32.shape[0]
    k32, w32 = k32.astype(np.float32), w32.astype(np.float32)
    tiles = []
    for c0 in range(0, n_keys, CHUNK):
        acc, used = np.zeros(k32.shape[1:], np.float32), False
        for i in range(c0, min(c0 + CHUNK, n_keys)):
            if w32[i] != 0:
                acc = (acc + (w32[i] * k32[i]).astype(np.float32)).astype(np.float32)
                used = True
        tiles.append((acc, used))
    if len(tiles) == 1:
        return tiles[0][0]
    out = np.zeros(k32.shape[1:], np.float32)
    for acc, used in tiles:
        if used:
            out = (out + acc).astype(np.float32)
    return out
