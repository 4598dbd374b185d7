"""Shared by ``test_refine_cpu.py`` and ``test_gpu_refine.py``: the refinement of soft word maps along an image's local colour
affinities (include/daam_refine.h) as a float64 numpy reference (weights and apply kept apart), a float32 emulation
in the kernels' operation order, the two error bounds, the images of the cases, and a numpy stand-in of ``libdaam_refine`` that
puts the Python layer under test without a GPU.  Test-only: the product has no fallback.

The error bounds (u = 2^-24, the unit roundoff of f32; K = 8 * len(dilations); all derived from the operations of
daam_refine.hip, none tuned on device output).

(a) Weights against float64: ``weights_bound``, an ABSOLUTE bound per weight.  The device forms, per channel, the exact integers
    S1 = sum v, S2 = sum v^2 over the n = K + 1 samples and V = n S2 - S1^2 (< 2^31), so sigma = sqrt(V) / (255 n) has no
    cancellation.  Roundings on the way to the logit a_k = -(1/C) sum_c |dI_c| / (1e-8 + s sigma_c), all on positive terms:
    float(V) u, sqrt u (half of its input's u carries over: 1.5 u so far), scale / (255 n) u, the fma with 1e-8f u (3.5 u),
    1 / (255 C) u and the division u (5.5 u), the first product and C - 1 fmas (8.5 u for C = 3); |dI| is an exact integer.  With
    slack for second-order terms: |a_k(device) - a_k| <= 10 u |a_k|.  The same maximum is subtracted from every logit, and a
    softmax does not change under a common shift, so the maximum's own error cancels; the subtraction rounds once, u |a_k - max| <=
    u |a_k| (max <= 0); expf is within 1 ulp = 2 u.  So e_k carries the relative error theta_k <= 11 u |a_k| + 2 u, rounded up here
    to 12 u |a_k| + 2 u.  The sum of K positive terms adds (K - 1) u and the division u.  A softmax's first-order response to
    relative errors theta_j of its terms is w_k (theta_k - sum_j w_j theta_j), hence

        |w_k(device) - w_k| <= w_k * (12 u (|a_k| + sum_j w_j |a_j|) + (K + 6) u) * (1 + 2^-9) + 2^-120.

    The relative error of a weight does grow with |a_k|, but a logit far below the maximum has w_k <= exp(-(max - a_k)), and
    x exp(-x) <= 1 / e: its ABSOLUTE error falls with it and needs no special case.  Where exp(a_k - max) leaves the normal range
    (max - a_k > 87) the device returns a subnormal or zero; both are within 2^-126 of the true weight, which the floor 2^-120
    covers.  (1 + 2^-9) covers exp(theta) - 1 <= theta (1 + theta) for theta < 2^-9, true of every |a_k| < 2700.

(b) Apply against float64 FED THE DEVICE'S WEIGHTS w^: ``apply_bound``.  One iteration is a K-term fma chain, so
    m^(p) = sum_k w^_k m(q_k) (1 + eta_k), |eta_k| <= g = K u / (1 - K u).  With S = max_p sum_k w^_k (taken from the device's weights
    in float64; 1 up to (a)) and M = max |m^0|, the error e_t after t iterations obeys e_{t+1} <= S e_t + g S max|m^_t| and
    max|m^_t| <= (S (1 + g))^t M, so

        e_T <= T g M (S (1 + g))^T        -- linear in T K 2^-24 max|m^0|.

    End to end against the pure float64 path (``combined_bound``): float64 iterations with w^ and with w differ by at most
    A M per iteration, A = max_p sum_k weights_bound_k(p), carried on with gain S: the bound is apply_bound + T A M max(S, 1)^T.
"""
import ctypes

import numpy as np

import _epilogue_domain as D
import _sweep_domain as S

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TILE = (4, 64)                              # rows x columns of a workgroup's tile (daam_refine.hip): one wave per row
OFFSETS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))          # (dy, dx)
DILATIONS = (1, 2, 4, 8, 12, 24)


def neighbours(h, w, dilations):
    """``(qy, qx)`` int [K, h, w]: the clamped neighbour coordinates, dilation-major, then ``OFFSETS``."""
    yy, xx = np.mgrid[0:h, 0:w]
    qy = np.stack([np.clip(yy + dy * d, 0, h - 1) for d in dilations for dy, _ in OFFSETS])
    qx = np.stack([np.clip(xx + dx * d, 0, w - 1) for d in dilations for _, dx in OFFSETS])
    return qy, qx


def _pixels(image):
    image = np.asarray(image)
    assert image.dtype == np.uint8
    return (image[:, :, None] if image.ndim == 2 else image).astype(np.int64)


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------
def logits64(image, dilations=DILATIONS, scale=0.1):
    """float64 [K, h, w]: a_k(p).  ``scale`` goes through f32, as the call's argument does."""
    px = _pixels(image)
    value = px / 255.0
    qy, qx = neighbours(px.shape[0], px.shape[1], dilations)
    near = value[qy, qx]                                                     # [K, h, w, C]
    sigma = np.concatenate([near, value[None]]).std(axis=0)                  # population
    return -(np.abs(near - value[None]) / (1e-8 + float(F32(scale)) * sigma)[None]).mean(axis=-1)


def softmax64(a):
    """Over axis 0, the maximum subtracted; the denominator is a compensated (Neumaier) sum, so that a weight carries the rounding
    of exp and of one division and the weights of a pixel sum to 1 within a few 2^-53."""
    e = np.exp(a - a.max(axis=0))
    total, lost = np.zeros_like(e[0]), np.zeros_like(e[0])
    for term in e:
        s = total + term
        lost += np.where(np.abs(total) >= np.abs(term), (total - s) + term, (term - s) + total)
        total = s
    return e / (total + lost)


def reference_weights(image, dilations=DILATIONS, scale=0.1):
    return softmax64(logits64(image, dilations, scale))


def reference_apply(weights, dilations, maps, iterations):
    """float64 [N, h, w]: ``iterations`` rounds of m(p) <- sum_k w_k(p) m(q_k(p)), ascending in k."""
    m = np.asarray(maps, F64)
    w = np.asarray(weights, F64)
    qy, qx = neighbours(m.shape[1], m.shape[2], dilations)
    for _ in range(iterations):
        acc = np.zeros_like(m)
        for k in range(w.shape[0]):
            acc += w[k] * m[:, qy[k], qx[k]]
        m = acc
    return m


def outputs(refined, threshold):
    """``(masks uint8 [N, h, w], labels uint8 [h, w])`` of f32 ``refined`` under the header's rules, compared in f32."""
    refined = np.asarray(refined, F32)
    masks = (refined > F32(threshold)).astype(np.uint8)
    owner = refined.argmax(axis=0)                                           # the first of equal maxima
    labels = np.where(refined.max(axis=0) > F32(threshold), owner, 255).astype(np.uint8)
    return masks, labels


def iou(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return (a & b).sum() / max((a | b).sum(), 1)


# ---- float32 emulation in the kernels' order -----------------------------------------------------------------------------------------
def fma32(a, b, c):
    """f32(a * b + c): the product of two f32 is exact in float64, so the only departure from a fused multiply-add is the double
    rounding of the sum (53 bits, then 24), which moves a result only when it lies within 2^-29 ulp of a tie."""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def emulate_weights(image, dilations=DILATIONS, scale=0.1):
    """f32 [K, h, w] in the operation order of refine_affinity_kernel (numpy's f32 exp stands for expf)."""
    px = _pixels(image)
    h, w, c = px.shape
    qy, qx = neighbours(h, w, dilations)
    near = px[qy, qx]
    n = near.shape[0] + 1
    s1, s2 = near.sum(axis=0) + px, (near * near).sum(axis=0) + px * px
    dev_scale, chan_scale = F32(F64(F32(scale)) / (255.0 * n)), F32(1.0 / (255.0 * c))
    r = chan_scale / fma32(dev_scale, np.sqrt((n * s2 - s1 * s1).astype(F32)), F32(1e-8))
    d = np.abs(near - px[None]).astype(F32)
    t = d[..., 0] * r[..., 0]
    for ch in range(1, c):
        t = fma32(d[..., ch], r[..., ch], t)
    a = -t
    e = np.exp((a - a.max(axis=0)).astype(F32)).astype(F32)
    total = e[0].copy()
    for k in range(1, e.shape[0]):
        total = total + e[k]
    return (e / total).astype(F32)


def emulate_apply(weights, dilations, maps, iterations):
    """f32 [N, h, w] in the order of refine_apply_kernel: acc = fma(w_k, m(q_k), acc) ascending in k from 0."""
    m, w = np.asarray(maps, F32), np.asarray(weights, F32)
    qy, qx = neighbours(m.shape[1], m.shape[2], dilations)
    for _ in range(iterations):
        acc = np.zeros_like(m)
        for k in range(w.shape[0]):
            acc = fma32(w[k][None], m[:, qy[k], qx[k]], acc)
        m = acc
    return m


# ---- bounds (module docstring) -------------------------------------------------------------------------------------------------------
def weights_bound(image, dilations=DILATIONS, scale=0.1):
    """float64 [K, h, w]: bound (a) on |w_k(device) - w_k(float64)|."""
    a = logits64(image, dilations, scale)
    w = softmax64(a)
    k = a.shape[0]
    spread = np.abs(a) + (w * np.abs(a)).sum(axis=0)[None]
    return w * (12 * U * spread + (k + 6) * U) * (1 + 2.0 ** -9) + 2.0 ** -120


def weight_sum(weights):
    return float(np.asarray(weights, F64).sum(axis=0).max())


def apply_bound(weights, maps, iterations):
    """Bound (b) on |refined(device) - float64 fed ``weights``| (the device's own)."""
    k = np.asarray(weights).shape[0]
    g = k * U / (1 - k * U)
    return iterations * g * float(np.abs(maps).max()) * (weight_sum(weights) * (1 + g)) ** iterations


def combined_bound(image, dilations, scale, weights, maps, iterations):
    """The end-to-end bound against the pure float64 path: (b) plus (a) carried through ``iterations`` rounds."""
    a = float(weights_bound(image, dilations, scale).sum(axis=0).max())
    return apply_bound(weights, maps, iterations) + iterations * a * float(np.abs(maps).max()) * max(weight_sum(weights), 1.0) ** iterations


# ---- images and maps -----------------------------------------------------------------------------------------------------------------
IMAGE_KINDS = ('flat', 'edge', 'random', 'pixel')


def image(kind, h, w, c, seed=0):
    """uint8 [h, w] (c == 1) or [h, w, 3]: flat; two regions with noise; uniform random bytes; one differing pixel."""
    rng = np.random.default_rng(seed)
    shape = (h, w) if c == 1 else (h, w, c)
    if kind == 'flat':
        out = np.full(shape, 137)
    elif kind == 'edge':
        yy, xx = np.mgrid[0:h, 0:w]
        side = (xx + 0.3 * yy > 0.45 * w)
        base = np.where(side, 190, 60)
        out = (base if c == 1 else base[:, :, None]) + rng.integers(-12, 13, shape)
    elif kind == 'random':
        out = rng.integers(0, 256, shape)
    else:
        out = np.full(shape, 100)
        out[h // 2, w // 3] = 220
    return np.clip(out, 0, 255).astype(np.uint8)


def maps(n, h, w, seed=0):
    """f32 [n, h, w] in [0, 1]: a bump per map plus noise; map 1 (if any) repeats map 0 so that the label rule meets ties."""
    rng = np.random.default_rng(seed + 1000)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for _ in range(n):
        cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), 0.25 * max(h, w) + 1
        out.append(0.8 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + 0.2 * rng.uniform(0, 1, (h, w)))
    out = np.stack(out).astype(F32)
    if n > 1:
        out[1] = out[0]
    return out


ELLIPSE = (45, 70)                          # image height, width
ELLIPSE_PLANE = (9, 14)                     # the word map's grid


def ellipse_case(seed=0):
    """``(image uint8 [45, 70, 3], truth bool [45, 70], plane f32 [9, 14])``: a noisy bright ellipse on a dark ground, and a word
    map that is a Gaussian shifted off the ellipse's centre -- a blob that ignores the outline."""
    h, w = ELLIPSE
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    truth = ((yy - 22) / 13.0) ** 2 + ((xx - 36) / 21.0) ** 2 <= 1.0
    img = np.where(truth, 200, 60)[:, :, None] + rng.normal(0, 8, (h, w, 3))
    py, px = np.mgrid[0:ELLIPSE_PLANE[0], 0:ELLIPSE_PLANE[1]]
    plane = np.exp(-(((py - 3.2) / 2.6) ** 2 + ((px - 5.6) / 3.6) ** 2) / 2)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), truth, plane.astype(F32)


def ellipse_soft(plane):
    """f32 [45, 70]: the plane as ``expand_as`` expands it (bicubic, min-max normalised), in the epilogue's emulation."""
    return D.emulate_expand(plane, *ELLIPSE)


# ---- a numpy stand-in of libdaam_refine ----------------------------------------------------------------------------------------------
class FakeRefineLib:
    """``daam_refine_affinity`` / ``daam_refine_apply`` and the two size functions in numpy (the f32 emulation) on CPU tensors'
    memory, held to the header's limits; records every call as ``('affinity', h, w, c, dilations, scale)`` or ``('apply', n_maps,
    h, w, dilations, iterations, threshold, masks asked for, labels asked for)``."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _size_ok(h, w, n_dil):
        return 1 <= n_dil <= 6 and h >= 1 and w >= 1 and 8 * n_dil * h * w < 2 ** 31

    def daam_refine_weights_bytes(self, h, w, n_dil):
        return 4 * 8 * n_dil * h * w if self._size_ok(h, w, n_dil) else 0

    def daam_refine_workspace(self, n_maps, h, w):
        return (4 * n_maps * h * w + 7) // 8 * 8 if 1 <= n_maps <= 32 and self._size_ok(h, w, 1) else 0

    @staticmethod
    def _dilations(dilations, n_dil):
        dil = tuple(int(d) for d in list(dilations)[:n_dil])
        assert 1 <= n_dil <= 6 and all(1 <= d <= 64 for d in dil) and all(b > a for a, b in zip(dil, dil[1:])), dil
        return dil

    def daam_refine_affinity(self, image, h, w, channels, dilations, n_dil, scale, weights, stream):
        dil = self._dilations(dilations, n_dil)
        assert image and weights and channels in (1, 3) and self._size_ok(h, w, n_dil) and np.isfinite(scale) and scale > 0
        self.calls.append(('affinity', h, w, channels, dil, float(F32(scale))))
        px = S._array(image, ctypes.c_uint8, h * w * channels).reshape(h, w, channels)
        S._array(weights, ctypes.c_float, 8 * n_dil * h * w)[:] = emulate_weights(px, dil, scale).ravel()
        return 0

    def daam_refine_apply(self, weights, dilations, n_dil, maps, n_maps, h, w, iterations, threshold, refined, masks, labels, ws, ws_bytes,
                          stream):
        dil = self._dilations(dilations, n_dil)
        assert weights and maps and refined and ws and ws_bytes >= self.daam_refine_workspace(n_maps, h, w) > 0
        assert self._size_ok(h, w, n_dil) and 0 <= iterations <= 64 and np.isfinite(threshold) and refined != maps
        self.calls.append(('apply', n_maps, h, w, dil, iterations, float(F32(threshold)), masks is not None, labels is not None))
        wt = S._array(weights, ctypes.c_float, 8 * n_dil * h * w).reshape(8 * n_dil, h, w)
        m = S._array(maps, ctypes.c_float, n_maps * h * w).reshape(n_maps, h, w)
        out = emulate_apply(wt, dil, m, iterations)
        S._array(refined, ctypes.c_float, n_maps * h * w)[:] = out.ravel()
        mk, lb = outputs(out, threshold)
        if masks is not None:
            S._array(masks, ctypes.c_uint8, n_maps * h * w)[:] = mk.ravel()
        if labels is not None:
            S._array(labels, ctypes.c_uint8, h * w)[:] = lb.ravel()
        return 0


def install(setattr_):
    """``_sweep_domain.install`` (CPU tensors pass for device tensors, ``engine.word_maps`` in torch) plus a ``FakeRefineLib`` under
    ``daam_amd.engine`` and ``engine.expand_word_map`` in numpy (``_epilogue_domain.emulate_expand``).  Returns ``(engine module,
    lib)``."""
    import torch
    E, _ = S.install(setattr_)
    lib = FakeRefineLib()
    setattr_(E.nat, 'load_refine', lambda: lib)

    def expand_word_map(word, out_h, out_w, absolute=False, threshold=None):
        return torch.from_numpy(D.emulate_expand(word.numpy(), out_h, out_w, absolute=absolute, threshold=threshold))
    setattr_(E, 'expand_word_map', expand_word_map)
    return E, lib
