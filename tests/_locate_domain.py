"""Shared by ``test_localize_cpu.py`` and ``test_gpu_localize.py``: the cases of ``daam_localize`` (include/daam_locate.h, DESIGN
3.19) -- those of ``_sweep_domain`` plus a few planes and truth masks of its own --, a numpy restatement of what it returns (from
the row and column maxima, as the kernels do) beside a brute-force one (from the masks), the float64 boxes of
``_epilogue_domain.expand``, and a numpy stand-in of ``libdaam_locate`` that puts the Python layer under test without a GPU.
Test-only: the product has no fallback."""
import ctypes

import numpy as np

import _epilogue_domain as D
import _sweep_domain as S

F32 = np.float32
EPS = F32(1e-8)
BIG_SIZE = ((64, 64), (512, 768))          # more than one tile in both directions, more columns than one tile's 256


# ---- planes and truth masks of this file ---------------------------------------------------------------------------------------------
def two_peaks(h=9, w=11):
    """(plane, (y1, x2), (y2, x1)): equal maxima at (y1, x2) and (y2, x1) with y1 < y2 and x1 < x2 -- the first row with the maximum
    is y1 and the first column with it is x1, and (y1, x1) is no maximum.  The peak is (y1, x2), the lower row-major index."""
    plane = (np.arange(h * w, dtype=F32).reshape(h, w) % 7) / F32(16)
    (y1, x2), (y2, x1) = (2, w - 3), (h - 2, 1)
    plane[y1, x2] = plane[y2, x1] = F32(2)
    assert plane[y1, x1] < 2
    return plane, (y1, x2), (y2, x1)


def constant_plane(h=5, w=7, value=0.25):
    return np.full((h, w), value, F32)


def edge_truth(oh, ow):
    """uint8 [2, oh, ow]: an all-zero mask, and one with the single pixel of the last row and column set (to 128)."""
    out = np.zeros((2, oh, ow), np.uint8)
    out[1, oh - 1, ow - 1] = 128
    return out


# ---- numpy restatements ------------------------------------------------------------------------------------------------------------------
def enc(v):
    """``enc_ordered`` of daam_epilogue.h: int32 whose order is the floats' (and -0 < +0)."""
    i = np.ascontiguousarray(v, F32).view(np.int32)
    return np.where(i >= 0, i, i ^ np.int32(0x7fffffff))


def raw_of(planes, oh, ow):
    """f32 [W, oh, ow]: the raw resized values (``_epilogue_domain.emulate_resize``), the kernels' arithmetic in numpy."""
    return np.stack([D.emulate_resize(p, oh, ow) for p in planes]).astype(F32)


def q(v, lo, hi):
    """The mask kernel's normalisation in f32: ``(v - lo) / (hi - lo + 1e-8f)``."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return ((np.asarray(v, F32) - F32(lo)) / ((F32(hi) - F32(lo)) + EPS)).astype(F32)


def lo_hi(raw):
    """Exact minimum and maximum of one word's raw values, in ``enc`` order."""
    flat = raw.reshape(-1)
    e = enc(flat)
    return flat[e.argmin()], flat[e.argmax()]


def box_of(mask):
    """``[x0, y0, x1, y1]`` of a bool [h, w]; ``[w, h, -1, -1]`` when nothing is set."""
    ys, xs = np.flatnonzero(mask.any(1)), np.flatnonzero(mask.any(0))
    if not len(ys):
        return [mask.shape[1], mask.shape[0], -1, -1]
    return [int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])]


def mask_boxes(masks):
    return np.array([box_of(np.asarray(m) != 0) for m in masks], np.int32).reshape(-1, 4)


def restate(raw, thr, absolute, truth=None):
    """What ``daam_localize`` returns, the way it gets there: from the raw values [W, oh, ow] the row and column maxima, the
    minimum and the first arg-max in ``enc`` order; the maxima normalised and compared.  ``(boxes int32 [W, T, 4], peaks int32
    [W, 2], peak_values f32 [W, 3], truth_boxes int32 [G, 4] or None, hits uint8 [W, G] or None)``."""
    raw = np.asarray(raw, F32)
    thr = np.asarray(thr, F32).reshape(-1)
    n_w, oh, ow = raw.shape
    boxes, peaks, values = np.zeros((n_w, len(thr), 4), np.int32), np.zeros((n_w, 2), np.int32), np.zeros((n_w, 3), F32)
    for j in range(n_w):
        e = enc(raw[j])
        at = int(e.reshape(-1).argmax())                                      # the first of equals
        lo, hi = lo_hi(raw[j])
        rows = np.take_along_axis(raw[j], e.argmax(1)[:, None], 1)[:, 0]
        cols = np.take_along_axis(raw[j], e.argmax(0)[None, :], 0)[0]
        if not absolute:
            rows, cols = q(rows, lo, hi), q(cols, lo, hi)
        peaks[j] = (at % ow, at // ow)
        values[j] = (raw[j].reshape(-1)[at], lo, hi)
        for t, tau in enumerate(thr):
            ys, xs = np.flatnonzero(rows > tau), np.flatnonzero(cols > tau)
            boxes[j, t] = [xs[0], ys[0], xs[-1], ys[-1]] if len(ys) else [ow, oh, -1, -1]
    if truth is None:
        return boxes, peaks, values, None, None
    truth = np.asarray(truth)
    hits = np.array([[truth[g, peaks[j, 1], peaks[j, 0]] != 0 for g in range(len(truth))] for j in range(n_w)], np.uint8).reshape(n_w, len(truth))
    return boxes, peaks, values, mask_boxes(truth), hits


def brute_boxes(raw, thr, absolute):
    """int32 [W, T, 4]: the boxes of the masks themselves -- every pixel normalised and compared."""
    raw = np.asarray(raw, F32)
    out = np.zeros((raw.shape[0], len(thr), 4), np.int32)
    for j in range(raw.shape[0]):
        v = raw[j] if absolute else q(raw[j], *lo_hi(raw[j]))
        for t, tau in enumerate(np.asarray(thr, F32)):
            out[j, t] = box_of(v > tau)
    return out


def box_iou(a, b):
    """Brute force IoU of two inclusive boxes by painting them (small images only); an empty box scores 0."""
    if a[2] < a[0] or b[2] < b[0]:
        return F32(0)
    n = max(a[2], b[2]) + 1, max(a[3], b[3]) + 1
    pa, pb = np.zeros((n[1], n[0]), bool), np.zeros((n[1], n[0]), bool)
    pa[a[1]:a[3] + 1, a[0]:a[2] + 1] = True
    pb[b[1]:b[3] + 1, b[0]:b[2] + 1] = True
    return F32((pa & pb).sum() / (pa | pb).sum())


# ---- the float64 oracle -----------------------------------------------------------------------------------------------------------------
def oracle_boxes(plane, oh, ow, absolute, thr):
    """Per threshold the box of the pixels surely above it and the box of those plus the ambiguous ones, from
    ``_sweep_domain.oracle_intervals``: ``dict(ill, inner int32 [T, 4], outer int32 [T, 4], ambiguous [T, oh, ow])``."""
    o = S.oracle_intervals(plane, oh, ow, absolute, thr)
    return dict(ill=o['ill'], inner=mask_boxes(o['sure']), outer=mask_boxes(o['sure'] | o['ambiguous']), ambiguous=o['ambiguous'])


def contains(outer, inner):
    """Box ``outer`` contains box ``inner`` (an empty box lies inside everything)."""
    return inner[2] < inner[0] or (outer[0] <= inner[0] and outer[1] <= inner[1] and outer[2] >= inner[2] and outer[3] >= inner[3])


# ---- a numpy stand-in of libdaam_locate ----------------------------------------------------------------------------------------------------
class FakeLocateLib:
    """``daam_localize`` / ``_workspace`` in numpy on CPU tensors' memory, held to the header's limits; records every call's
    ``(n_words, n_truth, thresholds)``."""

    def __init__(self):
        self.calls = []

    def daam_localize_workspace(self, n_words, n_truth, n_thr, out_h, out_w):
        ok = (0 <= n_words <= 32 and 0 <= n_truth <= 32 and n_words + n_truth >= 1 and 0 <= n_thr <= 64 and out_h >= 1 and out_w >= 1
              and out_h * out_w < 2 ** 31)
        return 512 + (4 * n_words * (out_h + out_w) + 7) // 8 * 8 if ok else 0

    def daam_localize(self, word_maps, n_words, h, w, out_h, out_w, absolute, thr, n_thr, truth, n_truth, boxes, peaks, values,
                      truth_boxes, hits, ws, ws_bytes, stream):
        assert ws_bytes >= self.daam_localize_workspace(n_words, n_truth, n_thr, out_h, out_w) > 0 and ws and ws % 8 == 0
        assert 1 <= h <= 128 and 1 <= w <= 128
        thr = np.array(list(thr)[:n_thr], F32)
        assert np.isfinite(thr).all()
        assert (word_maps is None) == (peaks is None) == (values is None) == (n_words == 0)
        assert (truth is None) == (truth_boxes is None) == (n_truth == 0)
        assert (boxes is None) == (n_words * n_thr == 0) and (hits is None) == (n_words * n_truth == 0)
        self.calls.append((n_words, n_truth, [float(t) for t in thr]))
        masks = S._array(truth, ctypes.c_uint8, n_truth * out_h * out_w).reshape(n_truth, out_h, out_w) if n_truth else None
        if n_words:
            planes = S._array(word_maps, ctypes.c_float, n_words * h * w).reshape(n_words, h, w)
            b, p, v, tb, hi = restate(raw_of(planes, out_h, out_w), thr, bool(absolute), masks)
            if n_thr:
                S._array(boxes, ctypes.c_int32, n_words * n_thr * 4)[:] = b.ravel()
            S._array(peaks, ctypes.c_int32, n_words * 2)[:] = p.ravel()
            S._array(values, ctypes.c_float, n_words * 3)[:] = v.ravel()
            if n_truth:
                S._array(hits, ctypes.c_uint8, n_words * n_truth)[:] = hi.ravel()
        if n_truth:
            S._array(truth_boxes, ctypes.c_int32, n_truth * 4)[:] = mask_boxes(masks).ravel()
        return 0


def install(setattr_):
    """``_sweep_domain.install`` (CPU tensors pass for device tensors) plus a ``FakeLocateLib`` under ``daam_amd.engine`` /
    ``evaluate``.  Returns ``(engine module, lib)``."""
    E, _ = S.install(setattr_)
    lib = FakeLocateLib()
    setattr_(E.nat, 'load_locate', lambda: lib)
    return E, lib
