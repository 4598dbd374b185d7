"""Shared by ``test_self_affinity_cpu.py`` and ``test_gpu_self_affinity.py``: the self-attention affinity and the propagation of soft
maps along it (include/daam_self_affinity.h) as a float64 numpy reference, a float32 emulation in the kernels' operation
order (with the mutants that show the bounds can fail), the error bounds, the inputs of the cases, and a numpy stand-in of
``libdaam_selfaff`` that puts the Python layer under test without a GPU.  Test-only: the product has no fallback.

Inputs are f32 arrays [batch, heads, P, d] whose values are exactly representable in the call's dtype ('f16' or 'bf16').

The error bounds (u = 2^-24, the unit roundoff of f32; all derived from the operations of daam_self_affinity.hip, none tuned on
device output).

(a) ``sums`` of a chain of calls against float64 on the same fp16 / bf16 inputs: ``sums_bound``, ABSOLUTE per entry.  Per slice:
    the product of two fp16 or two bf16 values is exact in f32; an any-order f32 sum of d of them carries (d - 1) u A_ij with
    A_ij = scale sum_c |q_ic k_jc|.  The device forms the exponent (in base 2) as fma(raw, c, -(m c)), c = f32(scale log2 e):
    the rounding of c moves the argument by u |x_ij|, the fma's own rounding by u |x_ij - max_j x_ij| (the fma's result IS that
    difference); the shift -(m c) is the same number in the statistics and in the sums kernel, and a softmax does not change under a
    common shift, so its own rounding cancels.  With |x_ij| <= A_ij:  theta_ij = (d + 1) u A_ij + u |x_ij - max_j x_ij|, in natural
    units after the factor ln 2 log2 e = 1.  v_exp_f32 is within 1 ulp = 2 u.  So e_ij carries the relative error tau_ij = theta_ij
    + 2 u.  The row sum l_i: an any-order sum of P positive terms, (P - 1) u; the online walk rescales the running sum once per
    32-key step, each time by exp2 of a rounded difference D <= 0 (relative error of the carried part at most u |D| ln 2 + 2 u, weighted
    by 2^D <= 1: at most 3 u) plus a product and a sum (2 u): 5 u ceil(P / 32); the combination of the two lane halves and the
    reciprocal: 10 u with slack.  c_row = (P - 1) + 5 ceil(P / 32) + 10.  A softmax's first-order response to relative errors of
    its terms gives

        |p_ij(device) - p_ij| <= p_ij (tau_ij + sum_l p_il tau_il + c_row u) (1 + 2^-9)  +  2^-126

    (the floor: where exp2 leaves the normal range the device returns 0; (1 + 2^-9) covers exp(t) - 1 <= t (1 + t) for t < 2^-9).
    The slices are added with one fma each, S u acc_ij in all, and the call ends with fma(weight, acc, previous): |weight| times the
    above plus u |result|.  A chain of calls adds its calls' bounds.

(b) Propagation against float64 FED THE DEVICE'S OWN sums: ``propagate_bound``.  A row's numerator is a sum of P products whose depth,
    in the documented order, is D = ceil(P / 64) + 6 (a lane's fma chain, then the butterfly): relative to sum_j s_ij |m_j| <= r_i M
    it carries g = D u / (1 - D u).  The row sum r_i carries the same g, the division u.  One iteration therefore errs by at most
    G M_t with G = 2 g + 2 u, and since every step is a convex combination the errors add with gain 1:

        e_T <= T G M (1 + G)^T,     M = max |m^0|.

(c) End to end against the pure float64 path: ``combined_bound``.  With delta_ij the bound (a) and R_i = sum_j delta_ij, a step with
    the device's sums differs from one with the exact sums by at most A M, A = max_i 2 R_i / (r_i - R_i); the bound is (b) + T A M (1 + A)^T.
"""
import ctypes
import math

import numpy as np
import torch

import _sweep_domain as S

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TILE = 128                                  # rows and columns of a tile of sums, rows of a statistics block
HEAD_DIMS = (40, 64, 80, 160)
LOG2E = 1.4426950408889634
DAAM_F16, DAAM_BF16 = 0, 2
E_INVALID = -1


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def quantize(x, dtype):
    """f32 array whose values are exactly those of ``x`` rounded to 'f16' or 'bf16'."""
    t = torch.from_numpy(np.ascontiguousarray(x, F32))
    return t.to(torch.float16 if dtype == 'f16' else torch.bfloat16).float().numpy()


def bits(x, dtype):
    """uint16 array: the device representation of a quantized f32 array."""
    t = torch.from_numpy(np.ascontiguousarray(x, F32)).to(torch.float16 if dtype == 'f16' else torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


REGIMES = ('small', 'peaked', 'outlier', 'zero_q')


def inputs(regime, batch, heads, P, d, dtype, seed=0):
    """``(q, k, scale)``: small logits; logits of about +-60 (a peaked softmax); one outlier key; an all-zero Q."""
    rng = np.random.default_rng(seed * 7919 + P * 31 + d)
    q = rng.standard_normal((batch, heads, P, d))
    k = rng.standard_normal((batch, heads, P, d))
    scale = d ** -0.5
    if regime == 'peaked':
        k = q[:, :, ::-1].copy() + 0.1 * k          # key P-1-i matches query i: x = scale |q|^2 ~ sqrt(d) * ... scaled below to ~60
        q = q * (60.0 / math.sqrt(d)) ** 0.5
        k = k * (60.0 / math.sqrt(d)) ** 0.5
    elif regime == 'outlier':
        q, k = 0.5 * q, 0.5 * k
        k[:, :, P // 2] = 4.0 * np.sign(q.mean(axis=2)) + 0.0 * k[:, :, P // 2]
    elif regime == 'zero_q':
        q = np.zeros_like(q)
    else:
        q, k = 0.5 * q, 0.5 * k
    return quantize(q, dtype), quantize(k, dtype), float(F32(scale))


def maps(n, P, seed=0, signed=False):
    rng = np.random.default_rng(seed + 500)
    m = rng.uniform(-1 if signed else 0, 1, (n, P))
    return m.astype(F32)


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------
def logits64(q, k, scale):
    return float(F32(scale)) * np.einsum('bhic,bhjc->bhij', q.astype(F64), k.astype(F64))


def softmax64(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def reference_sums(calls, prior=None):
    """float64 [P, P]: ``calls`` is a sequence of ``(q, k, scale, weight)``; the first call overwrites (``accumulate == 0``) unless
    ``prior`` is given."""
    out = None if prior is None else np.asarray(prior, F64)
    for q, k, scale, weight in calls:
        acc = softmax64(logits64(q, k, scale)).sum(axis=(0, 1))
        out = float(F32(weight)) * acc + (0.0 if out is None else out)
    return out


def reference_propagate(sums, m, iterations, normalise=True):
    s, m = np.asarray(sums, F64), np.asarray(m, F64)
    r = s.sum(axis=1)
    for _ in range(iterations):
        num = m @ s.T
        m = np.where(r == 0, m, num / np.where(r == 0, 1, r)) if normalise else num
    return m


# ---- float32 emulation ---------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def _acc_rows(half):
    return [(reg & 3) + 8 * (reg >> 2) + 4 * half for reg in range(16)]


def emulate_stats(raw, c, count_padded=False):
    """``(negm, rinv)`` f32 [P] of one slice's raw dot products f32 [P, P]: the maximum, then per lane half the 16-term partial sums
    of every 32-key step in register order, the steps added ascending, the lower half first.  (The device rescales a running sum
    where this uses the final maximum: the bound covers either.)"""
    P = raw.shape[0]
    negm = -(raw.max(axis=1) * c).astype(F32)
    pad = -(-P // 32) * 32
    y = np.full((P, pad), -np.inf, F32)
    y[:, :P] = fma32(raw, c, negm[:, None])
    if count_padded:
        y[:, P:] = negm[:, None]                     # a zero-filled key: raw = 0
    e = np.exp2(y).astype(F32).reshape(P, pad // 32, 32)
    halves = []
    for half in (0, 1):
        total = np.zeros(P, F32)
        for t in range(pad // 32):
            part = np.zeros(P, F32)
            for row in _acc_rows(half):
                part = part + e[:, t, row]
            total = total + part
        halves.append(total)
    return negm, (F32(1) / (halves[0] + halves[1])).astype(F32)


def emulate_sums(calls, prior=None, mutant=None):
    """f32 [P, P] in the order of the two kernels.  ``mutant``: 'no_scale', 'padded_keys', 'neighbour_stats', 'packed_head_stride'."""
    out = None if prior is None else np.asarray(prior, F32)
    for q, k, scale, weight in calls:
        b, h, P, d = q.shape
        c = F32(LOG2E if mutant == 'no_scale' else F64(F32(scale)) * LOG2E)
        if mutant == 'packed_head_stride':            # [b, P, h d] memory read as if it were [b, h, P, d]
            q = q.transpose(0, 2, 1, 3).reshape(b, h, P, d)
            k = k.transpose(0, 2, 1, 3).reshape(b, h, P, d)
        acc = np.zeros((P, P), F32)
        for s in range(b * h):
            raw = (q[s // h, s % h].astype(F64) @ k[s // h, s % h].astype(F64).T).astype(F32)
            negm, rinv = emulate_stats(raw, c, count_padded=mutant == 'padded_keys')
            if mutant == 'neighbour_stats':
                negm, rinv = np.roll(negm, -1), np.roll(rinv, -1)
            acc = fma32(np.exp2(fma32(raw, c, negm[:, None])).astype(F32), rinv[:, None], acc)
        out = fma32(F32(weight), acc, F32(0) if out is None else out)
    return out


def wave_sum(partials):
    """The butterfly of the kernels over f32 [..., 64]: lane distances 32 .. 1; every lane ends with the same bits."""
    v = np.asarray(partials, F32)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ off]
    return v[..., 0]


def emulate_propagate(sums, m, iterations, mutant=None):
    """f32 [N, P] in the kernels' order.  ``mutant``: 'no_normalisation'."""
    s, m = np.asarray(sums, F32), np.asarray(m, F32)
    P = s.shape[0]
    steps = -(-P // 64)
    sp = np.zeros((P, steps * 64), F32)
    sp[:, :P] = s
    sp = sp.reshape(P, steps, 64)
    part = np.zeros((P, 64), F32)
    for t in range(steps):
        part = part + sp[:, t]
    r = wave_sum(part)
    for _ in range(iterations):
        mp = np.zeros((m.shape[0], steps * 64), F32)
        mp[:, :P] = m
        mp = mp.reshape(m.shape[0], steps, 64)
        acc = np.zeros((m.shape[0], P, 64), F32)
        for t in range(steps):
            acc = fma32(sp[None, :, t], mp[:, None, t], acc)
        num = wave_sum(acc)
        if mutant == 'no_normalisation':
            m = num
        else:
            with np.errstate(divide='ignore', invalid='ignore'):
                m = np.where(r[None] == 0, m, (num / r[None]).astype(F32))
    return m


# ---- bounds (module docstring) -------------------------------------------------------------------------------------------------------
def sums_bound(calls, prior_bound=None, prior=None):
    """float64 [P, P]: bound (a) on |sums(device) - reference_sums(calls)|."""
    bound = 0.0 if prior_bound is None else np.asarray(prior_bound, F64)
    value = None if prior is None else np.asarray(prior, F64)
    for q, k, scale, weight in calls:
        b, h, P, d = q.shape
        sc, w = float(F32(scale)), abs(float(F32(weight)))
        x = logits64(q, k, scale)
        a = sc * np.einsum('bhic,bhjc->bhij', np.abs(q).astype(F64), np.abs(k).astype(F64))
        p = softmax64(x)
        tau = (d + 1) * U * a + U * np.abs(x - x.max(axis=-1, keepdims=True)) + 2 * U
        c_row = (P - 1) + 5 * -(-P // 32) + 10
        per = p * (tau + (p * tau).sum(axis=-1, keepdims=True) + c_row * U) * (1 + 2.0 ** -9) + 2.0 ** -126
        acc = p.sum(axis=(0, 1))
        value = float(F32(weight)) * acc + (0.0 if value is None else value)
        bound = bound + w * (per.sum(axis=(0, 1)) + b * h * U * acc) + U * np.abs(value) * (1 + 2.0 ** -9)
    return bound


def propagate_bound(P, m, iterations):
    depth = -(-P // 64) + 6
    g = depth * U / (1 - depth * U)
    G = 2 * g + 2 * U
    return iterations * G * float(np.abs(m).max()) * (1 + G) ** iterations


def combined_bound(delta, sums64, m, iterations):
    """Bound (c): ``delta`` is bound (a) per entry, ``sums64`` the exact sums."""
    R, r = np.asarray(delta, F64).sum(axis=1), np.asarray(sums64, F64).sum(axis=1)
    ok = r > R
    A = float((2 * R[ok] / (r[ok] - R[ok])).max()) if ok.any() else 0.0
    return propagate_bound(len(r), m, iterations) + iterations * A * float(np.abs(m).max()) * (1 + A) ** iterations


# ---- the block-structured case of the Python layer -------------------------------------------------------------------------------------
BLOCK_GRID = (45, 70)


def block_case(seed=0, d=40, dtype='f16'):
    """``(q = k f32 [1, 1, P, d], truth bool [45, 70], plane f32 [45, 70])``: a two-valued feature per cell (an ellipse and its ground)
    plus noise, so that the affinity is block-structured, and a word map that is a Gaussian shifted off the ellipse."""
    h, w = BLOCK_GRID
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    truth = ((yy - 22) / 13.0) ** 2 + ((xx - 36) / 21.0) ** 2 <= 1.0
    a, b = rng.standard_normal(d), rng.standard_normal(d)
    feat = np.where(truth.reshape(-1, 1), a[None], b[None]) * 1.5 + 0.3 * rng.standard_normal((h * w, d))
    plane = np.exp(-(((yy - 14) / 11.0) ** 2 + ((xx - 27) / 17.0) ** 2) / 2)
    qk = quantize(feat[None, None], dtype)
    return qk, truth, plane.astype(F32)


def iou(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return (a & b).sum() / max((a | b).sum(), 1)


# ---- a numpy stand-in of libdaam_selfaff ---------------------------------------------------------------------------------------------
class FakeSelfAffinityLib:
    """The four entry points in numpy (the f32 emulation) on CPU tensors' memory, held to the header's limits; records every call as
    ``('accumulate', dtype, batch, heads, P, d, strides, scale, weight, accumulate)`` or ``('propagate', P, N, iterations)``."""

    def __init__(self):
        self.calls = []

    def daam_self_affinity_workspace(self, batch, heads, P):
        ok = batch >= 1 and heads >= 1 and batch * heads <= 4096 and 1 <= P <= 16384
        return 8 * batch * heads * (-(-P // TILE) * TILE) if ok else 0

    def daam_self_affinity_propagate_workspace(self, N, P):
        return (4 * (N + 1) * P + 7) // 8 * 8 if 1 <= N <= 32 and 1 <= P <= 16384 else 0

    def daam_self_affinity_accumulate(self, q, k, dtype, batch, heads, P, d, qsb, qsh, qsp, ksb, ksh, ksp, scale, weight, accumulate, sums,
                                      ws, ws_bytes, stream):
        assert q and k and sums and ws and dtype in (DAAM_F16, DAAM_BF16) and d in HEAD_DIMS
        assert ws_bytes >= self.daam_self_affinity_workspace(batch, heads, P) > 0
        assert all(s >= 0 and s % 8 == 0 for s in (qsb, qsh, qsp, ksb, ksh, ksp)) and q % 16 == 0 and k % 16 == 0
        assert math.isfinite(scale) and scale > 0 and math.isfinite(weight)
        self.calls.append(('accumulate', dtype, batch, heads, P, d, (qsb, qsh, qsp, ksb, ksh, ksp), float(F32(scale)), float(F32(weight)),
                           int(accumulate)))

        def gather(ptr, sb, sh, sp):
            n = (batch - 1) * sb + (heads - 1) * sh + (P - 1) * sp + d
            raw = torch.from_numpy(S._array(ptr, ctypes.c_int16, n).copy())
            vals = raw.view(torch.float16 if dtype == DAAM_F16 else torch.bfloat16).float().numpy()
            return np.lib.stride_tricks.as_strided(vals, (batch, heads, P, d), tuple(4 * s for s in (sb, sh, sp, 1))).copy()
        out = S._array(sums, ctypes.c_float, P * P).reshape(P, P)
        out[:] = emulate_sums([(gather(q, qsb, qsh, qsp), gather(k, ksb, ksh, ksp), scale, weight)], prior=out.copy() if accumulate else None)
        return 0

    def daam_self_affinity_propagate(self, sums, P, m, N, iterations, refined, ws, ws_bytes, stream):
        assert sums and m and refined and ws and refined != m and 0 <= iterations <= 16
        assert ws_bytes >= self.daam_self_affinity_propagate_workspace(N, P) > 0
        self.calls.append(('propagate', P, N, iterations))
        s = S._array(sums, ctypes.c_float, P * P).reshape(P, P)
        src = S._array(m, ctypes.c_float, N * P).reshape(N, P)
        S._array(refined, ctypes.c_float, N * P)[:] = emulate_propagate(s, src, iterations).ravel()
        return 0


def install(setattr_):
    """``_sweep_domain.install`` (CPU tensors pass for device tensors) plus a ``FakeSelfAffinityLib`` under ``daam_amd.engine``.
    Returns ``(engine module, lib)``."""
    E, _ = S.install(setattr_)
    lib = FakeSelfAffinityLib()
    setattr_(E.nat, 'load_self_affinity', lambda: lib)
    setattr_(E, '_check_on_device', lambda query, key: None)
    return E, lib
