"""Shared by ``test_threshold_sweep_cpu.py`` and ``test_gpu_threshold_sweep.py``: the cases of the threshold sweep
(``daam_threshold_sweep``, include/daam_eval.h), a numpy restatement of what it counts, the float64 intervals of
``_epilogue_domain.expand`` for those counts, and a numpy stand-in of ``libdaam_eval`` that puts the Python layer under test without
a GPU.  Test-only: the product has no fallback.

Thresholds of the oracle cases.  A min-max normalised plane takes the value 0 at its minimum and (nearly) 1 at its maximum, so
one pixel each is ambiguous at the thresholds 0.0 and 1.0: those two are swept only where a case has at least 1000 pixels (one
pixel is then within the cap of 2e-3).  The ``peak_last`` / ``peak_first`` planes are constant but for one corner: after min-max
their whole background lies at 0 resp. 1, and unnormalised at 0.25, so they are swept at thresholds away from those three."""
import contextlib
import ctypes

import numpy as np
import torch

import _epilogue_domain as D

F32 = np.float32
SIZES = D.MASK_SIZES + [((12, 20), (12, 20)), ((48, 48), (32, 32))]     # + identity, down; (64,64)->(200,333): widths % 4 != 0, 66 workgroups
FULL_SIZE = ((16, 24), (37, 53))
# (words, truth masks, thresholds): every W of {1, 3, 32}, G of {0, 1, 5, 32}, T of {1, 2, 21, 64}
COMBOS = [(1, 0, 1), (3, 1, 2), (32, 5, 21), (3, 32, 64), (1, 5, 64), (32, 0, 2), (3, 5, 21), (32, 1, 1)]
WORD_KINDS = D.MASK_KINDS + ('real', 'levels')


def thresholds(n):
    """``n`` ascending f32 thresholds: 1 -> 0.4; 2 -> the ends 0 and 1; 21 -> the default i / 20; 64 -> -0.25, 0, 0.4, 1, 1.5 and
    59 more between -0.1 and 1.1."""
    if n == 1:
        return [0.4]
    if n == 2:
        return [0.0, 1.0]
    if n == 21:
        return [i / 20 for i in range(21)]
    fixed = [-0.25, 0.0, 0.4, 1.0, 1.5]
    rest = [float(F32(-0.1 + 1.2 * (i + 0.37) / (n - len(fixed)))) for i in range(n - len(fixed))]
    out = sorted(set(float(F32(t)) for t in fixed + rest))
    assert len(out) == n
    return out


def word_planes(n, h, w, seed=0):
    """f32 [n, h, w]: word j is a plane of kind ``WORD_KINDS[j % 7]``."""
    return np.stack([D.word_plane(WORD_KINDS[j % len(WORD_KINDS)], h, w, seed + j) for j in range(n)])


def truth_stack(g, oh, ow, seed=0):
    """uint8 [g, oh, ow]: mask i is a random rectangle thinned to about two thirds, its set bytes 1, 2, 128 or 255."""
    rng = np.random.default_rng([seed, g, oh, ow, 7])
    out = np.zeros((g, oh, ow), np.uint8)
    for i in range(g):
        y0, x0 = rng.integers(0, max(oh // 2, 1)), rng.integers(0, max(ow // 2, 1))
        y1, x1 = rng.integers(y0 + 1, oh + 1), rng.integers(x0 + 1, ow + 1)
        box = out[i, y0:y1, x0:x1]
        box[...] = np.where(rng.random(box.shape) < 2 / 3, rng.choice(np.array([1, 2, 128, 255], np.uint8), box.shape), 0)
    return out


def counts(values, thr, truth=None):
    """What the sweep counts, from the f32 values [W, oh, ow] it compares: ``(pred_area [W, T], inter [W, G, T], truth_area [G])``
    int64 -- the bin of a pixel is ``#{t : v > f32(thr[t])}`` (NaN: 0), the outputs are suffix sums of the per-bin counts."""
    thr = np.asarray(thr, F32)
    assert (np.diff(thr) > 0).all()
    values = np.asarray(values, F32)
    n_w, n_t = values.shape[0], len(thr)
    with np.errstate(invalid='ignore'):
        bins = (values[..., None] > thr).sum(-1)                               # [W, oh, ow] in 0..T
    sets = np.zeros((0,) + values.shape[1:], bool) if truth is None else np.asarray(truth) != 0
    pred, inter = np.zeros((n_w, n_t), np.int64), np.zeros((n_w, len(sets), n_t), np.int64)
    for j in range(n_w):
        hist = np.bincount(bins[j].ravel(), minlength=n_t + 1)
        pred[j] = hist[::-1].cumsum()[::-1][1:]
        for g, s in enumerate(sets):
            hist = np.bincount(bins[j][s], minlength=n_t + 1)
            inter[j, g] = hist[::-1].cumsum()[::-1][1:]
    return pred, inter, sets.sum((1, 2))


def values_of(planes, oh, ow, absolute):
    """f32 [W, oh, ow]: ``_epilogue_domain.emulate_expand`` of every plane -- the kernels' arithmetic in numpy."""
    return np.stack([D.emulate_expand(p, oh, ow, absolute=absolute) for p in planes]).astype(F32)


# ---- the float64 oracle ----------------------------------------------------------------------------------------------------------------
ORACLE_FULL = (-0.25, 0.0, 0.1, 0.4, 0.55, 0.9, 1.0, 1.5)
ORACLE_INNER = (-0.25, 0.1, 0.4, 0.55, 0.9, 1.5)
ORACLE_GROUPS = (('negative', 'signed', 'tiny'), ('peak_last', 'peak_first'))
assert sorted(k for g in ORACLE_GROUPS for k in g) == sorted(D.MASK_KINDS)


def oracle_cases():
    """(sizes, kinds of the call's words, absolute, thresholds) of every call the GPU file holds to the float64 oracle."""
    for sizes in SIZES:
        for kinds in ORACLE_GROUPS:
            for absolute in (False, True):
                big = sizes[1][0] * sizes[1][1] >= 1000
                yield sizes, kinds, absolute, ORACLE_FULL if big and kinds == ORACLE_GROUPS[0] else ORACLE_INNER


def oracle_planes(sizes, kinds):
    return np.stack([D.word_plane(k, *sizes[0], seed=3 + i) for i, k in enumerate(kinds)])


def oracle_intervals(plane, oh, ow, absolute, thr, truth=None):
    """Per threshold: the pixels surely above it and the ambiguous ones (``|want - f32(t)| <= bound``), from
    ``_epilogue_domain.expand``: ``dict(ill, sure [T, oh, ow] bool, ambiguous [T, oh, ow] bool)``."""
    ref = D.expand(plane, oh, ow, absolute=absolute)
    val, bound = ref['value'], ref['value_bound']
    t64 = np.asarray(thr, F32).astype(np.float64)[:, None, None]
    amb = (np.abs(val[None] - t64) <= bound[None]) & (bound[None] > 0)
    return dict(ill=ref['ill'], sure=(val[None] > t64) & ~amb, ambiguous=amb)


# ---- a numpy stand-in of libdaam_eval ----------------------------------------------------------------------------------------------------
def _array(ptr, ctype, n):
    return np.ctypeslib.as_array((ctype * n).from_address(int(ptr))) if n else np.zeros(0, ctype)


class FakeEvalLib:
    """``daam_threshold_sweep`` / ``_workspace`` in numpy on CPU tensors' memory, held to the header's limits; records every call's
    ``(n_words, n_truth, thresholds)``."""

    def __init__(self):
        self.calls = []

    def daam_threshold_sweep_workspace(self, n_words, n_truth, n_thr, out_h, out_w):
        ok = 1 <= n_words <= 32 and 0 <= n_truth <= 32 and 1 <= n_thr <= 64 and out_h >= 1 and out_w >= 1 and out_h * out_w < 2 ** 31
        return 256 + 4 * n_words * (n_thr + 1) * (n_truth + 1) if ok else 0

    def daam_threshold_sweep(self, word_maps, n_words, h, w, out_h, out_w, absolute, thr, n_thr, truth, n_truth, pred, inter, area,
                             ws, ws_bytes, stream):
        assert ws_bytes >= self.daam_threshold_sweep_workspace(n_words, n_truth, n_thr, out_h, out_w) > 0 and ws
        assert 1 <= h <= 128 and 1 <= w <= 128
        thr = np.array(list(thr)[:n_thr], F32)
        assert np.isfinite(thr).all() and (np.diff(thr) > 0).all(), thr
        assert (truth is None) == (inter is None) == (area is None) == (n_truth == 0)
        self.calls.append((n_words, n_truth, [float(t) for t in thr]))
        planes = _array(word_maps, ctypes.c_float, n_words * h * w).reshape(n_words, h, w)
        masks = _array(truth, ctypes.c_uint8, n_truth * out_h * out_w).reshape(n_truth, out_h, out_w) if n_truth else None
        p, i, a = counts(values_of(planes, out_h, out_w, bool(absolute)), thr, masks)
        _array(pred, ctypes.c_int32, n_words * n_thr)[:] = p.ravel()
        if n_truth:
            _array(inter, ctypes.c_int32, n_words * n_truth * n_thr)[:] = i.ravel()
            _array(area, ctypes.c_int32, n_truth)[:] = a
        return 0


class _Stream:
    cuda_stream = 0


def install(setattr_):
    """Put a ``FakeEvalLib`` under ``daam_amd.engine`` / ``evaluate`` through ``setattr_`` (``monkeypatch.setattr``) and let CPU tensors
    pass for device tensors; ``engine.word_maps`` becomes the mean of the planes in torch.  Returns ``(engine module, lib)``."""
    from daam_amd import engine as E, evaluate as ev
    lib = FakeEvalLib()
    setattr_(E.nat, 'load_eval', lambda: lib)
    setattr_(E, '_check_maps', lambda maps: None)
    setattr_(E, 'word_maps', lambda maps, idx_lists: torch.stack([maps[list(i)].mean(0) for i in idx_lists]).contiguous())
    setattr_(ev, '_to_hip', lambda t, name, device=None: t)
    setattr_(torch.cuda, 'device', lambda d: contextlib.nullcontext())
    setattr_(torch.cuda, 'current_stream', lambda d=None: _Stream())
    return E, lib
