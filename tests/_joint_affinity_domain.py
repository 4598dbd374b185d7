"""Shared by ``test_joint_affinity_cpu.py`` and ``test_gpu_joint_affinity.py``: the image columns of the joint softmax
(include/daam_joint_affinity.h) as a float64 numpy reference, a float32 emulation in the kernel's operation order (with
the mutants that show the bound can fail), the error bound, and numpy stand-ins of ``libdaam_jointaff`` and of a ``libdaam_joint``
that leaves its statistics in the workspace, which put the Python layer under test without a GPU.  Test-only: the product has no
fallback.  Inputs, logits, the softmax, the statistics' emulation and u are those of ``_joint_domain``.

A call is ``(q, k_txt, k_img, scale, weight)`` with f32 arrays q [batch, heads, P, d], k_txt [batch, heads, T, d], k_img
[batch, heads, Pk, d] whose values are exactly representable in the call's dtype.  The result is [P, Pk], query-major.

The error bound, ``sums_bound``: ABSOLUTE per entry of ``sums`` of a chain of calls against float64 on the same inputs.  It is the
per-entry term of ``_joint_domain.sums_bound`` -- whose derivation holds for ANY column of the joint softmax, the image kernel forms
exp2(fma(raw, c, -(m c))) * (1 / l) from the same raw f32 dot products (any-order sums of d exact products) and the same statistics
as the text kernel -- taken over the IMAGE columns:

    |p_ij(device) - p_ij| <= p_ij (tau_ij + sum_l p_il tau_il + c_row u) (1 + 2^-9)  +  2^-126

with tau_ij = (d + 1) u A_ij + u |x_ij - max_j x_ij| + 2 u, the sum over l over ALL T + Pk keys and
c_row = (T + Pk - 1) + 5 (ceil(T / 32) + ceil(Pk / 32)) + 10 exactly as there; the matrix adds its S = batch heads slices with one
fma each, S u acc in all; the call ends with fma(weight, acc, previous): |weight| times the above plus u |result|.  A chain of calls
adds its calls' bounds.
"""
import ctypes
import math

import numpy as np
import torch

import _joint_domain as J
import _sweep_domain as S
from _joint_domain import U, emulate_stats, fma32, inputs, logits64, softmax64  # noqa: F401  (re-exported to the tests)

F32, F64 = np.float32, np.float64
TILE = 128
LOG2E = J.LOG2E
DAAM_F16, DAAM_BF16 = J.DAAM_F16, J.DAAM_BF16
E_INVALID = -1


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
PS = (1, 5, 63, 65, 130, 257)                         # inside one tile on either side of an MFMA block and of a wave's 64; two and three tiles
TS = (1, 77, 154)
REGIMES = J.REGIMES

# (P, T, Pk, d, dtype, (batch, heads), layout, regime): every P x head dim x dtype with Pk = P; T, slice counts, layouts and regimes
# rotate so that each value meets both head dims and both dtypes.  Then Pk != P either way, once per head dim.
CASES = [(P, TS[(pi + di + ti) % 3], P, d, dtype, J.SLICES[(pi + di + ti) % 3], J.LAYOUTS[(pi + di) % 2], REGIMES[(pi + di + 2 * ti) % 4])
         for pi, P in enumerate(PS) for di, d in enumerate(J.HEAD_DIMS) for ti, dtype in enumerate(('f16', 'bf16'))]
CASES += [(65, 77, 200, 64, 'bf16', (1, 3), 'packed', 'outlier'), (200, 154, 65, 128, 'f16', (2, 3), 'interleaved', 'small')]


def case_id(c):
    return f'P{c[0]}-T{c[1]}-Pk{c[2]}-d{c[3]}-{c[4]}-S{c[5][0]}x{c[5][1]}-{c[6]}-{c[7]}'


def case_inputs(c, regime=None):
    P, T, Pk, d, dtype, (batch, heads) = c[:6]
    return inputs(regime or c[7], batch, heads, P, T, Pk, d, dtype, seed=P + T + d)


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------
def reference_sums(calls, prior=None):
    """float64 [P, Pk]: the image columns of the joint softmax summed over slices; the first call overwrites unless ``prior``."""
    out = None if prior is None else np.asarray(prior, F64)
    for q, kt, ki, scale, weight in calls:
        acc = softmax64(logits64(q, kt, ki, scale))[..., kt.shape[2]:].sum(axis=(0, 1))
        out = float(F32(weight)) * acc + (0.0 if out is None else out)
    return out


def text_mass(calls):
    """float64 [P]: the mass the cells gave to the text keys, summed over slices and calls (weights taken as 1)."""
    return sum(softmax64(logits64(q, kt, ki, scale))[..., :kt.shape[2]].sum(axis=(0, 1, 3)) for q, kt, ki, scale, _ in calls)


# ---- bound (module docstring) --------------------------------------------------------------------------------------------------------
def sums_bound(calls, prior_bound=None, prior=None):
    bound = 0.0 if prior_bound is None else np.asarray(prior_bound, F64)
    value = None if prior is None else np.asarray(prior, F64)
    for q, kt, ki, scale, weight in calls:
        b, h, P, d = q.shape
        T, n = kt.shape[2], kt.shape[2] + ki.shape[2]
        sc, w = float(F32(scale)), abs(float(F32(weight)))
        x = logits64(q, kt, ki, scale)
        a = sc * np.einsum('bhic,bhjc->bhij', np.abs(q).astype(F64), np.abs(np.concatenate([kt, ki], axis=2)).astype(F64))
        p = softmax64(x)
        tau = (d + 1) * U * a + U * np.abs(x - x.max(axis=-1, keepdims=True)) + 2 * U
        steps = -(-T // 32) + -(-(n - T) // 32)
        c_row = (n - 1) + 5 * steps + 10
        per = p * (tau + (p * tau).sum(axis=-1, keepdims=True) + c_row * U) * (1 + 2.0 ** -9) + 2.0 ** -126
        acc = p[..., T:].sum(axis=(0, 1))
        value = float(F32(weight)) * acc + (0.0 if value is None else value)
        bound = bound + w * (per[..., T:].sum(axis=(0, 1)) + b * h * U * acc) + U * np.abs(value) * (1 + 2.0 ** -9)
    return bound


# ---- float32 emulation ---------------------------------------------------------------------------------------------------------------
def image_columns(raw_i, c, negm, rinv, acc):
    """One slice of the kernel: acc [P, Pk] f32 + exp2(fma(raw, c, negm)) * rinv, one fma per entry."""
    return fma32(np.exp2(fma32(raw_i, c, negm[:, None])).astype(F32), rinv[:, None], acc)


MUTANTS = ('no_text_keys', 'transposed', 'no_scale', 'neighbour_stats', 'padded_row_stride', 'packed_head_stride')


def emulate_sums(calls, prior=None, mutant=None):
    """f32 [P, Pk] in the order of the statistics kernel of the joint tap and of the image kernel.  ``mutant``: one of ``MUTANTS``."""
    out = None if prior is None else np.asarray(prior, F32)
    for q, kt, ki, scale, weight in calls:
        b, h, P, d = q.shape
        Pk = ki.shape[2]
        c = F32(LOG2E if mutant == 'no_scale' else F64(F32(scale)) * LOG2E)
        if mutant == 'packed_head_stride':            # [b, rows, h d] memory read as if it were [b, h, rows, d]
            q, kt, ki = (x.transpose(0, 2, 1, 3).reshape(x.shape) for x in (q, kt, ki))
        pad = -(-Pk // TILE) * TILE if mutant == 'padded_row_stride' else Pk
        acc = np.zeros((P, pad), F32)
        for s in range(b * h):
            qs = q[s // h, s % h].astype(F64)
            raw_t = (qs @ kt[s // h, s % h].astype(F64).T).astype(F32)
            raw_i = (qs @ ki[s // h, s % h].astype(F64).T).astype(F32)
            negm, rinv = emulate_stats(raw_t[:, :0] if mutant == 'no_text_keys' else raw_t, raw_i, c)
            if mutant == 'neighbour_stats':
                negm, rinv = np.roll(negm, -1), np.roll(rinv, -1)
            if pad != Pk:                             # the zero-filled keys past Pk: raw = 0
                raw_i = np.concatenate([raw_i, np.zeros((P, pad - Pk), F32)], axis=1)
            acc = image_columns(raw_i, c, negm, rinv, acc)
        if mutant == 'transposed':
            acc = np.ascontiguousarray(acc.T)
        if pad != Pk:                                 # rows `pad` floats apart in a buffer of P Pk floats, stores in row order
            flat = np.zeros(P * pad, F32)
            flat[:] = acc.ravel()
            acc = flat[:P * Pk].reshape(P, Pk)
        out = fma32(F32(weight), acc, F32(0) if out is None else out)
    return out


# ---- numpy stand-ins of the two libraries --------------------------------------------------------------------------------------------
def _gather(ptr, dtype, batch, heads, rows, d, sb, sh, sp):
    if not rows:
        return np.zeros((batch, heads, 0, d), F32)
    n = (batch - 1) * sb + (heads - 1) * sh + (rows - 1) * sp + d
    raw = torch.from_numpy(S._array(ptr, ctypes.c_int16, n).copy())
    vals = raw.view(torch.float16 if dtype == DAAM_F16 else torch.bfloat16).float().numpy()
    return np.lib.stride_tricks.as_strided(vals, (batch, heads, rows, d), tuple(4 * s for s in (sb, sh, sp, 1))).copy()


class FakeJointLibWithStats(J.FakeJointLib):
    """``_joint_domain.FakeJointLib`` that, like the device library of ABI 1, leaves ``(-(m c), 1 / l)`` of every query row in the
    workspace, slices pad128(P) rows apart; ``ptrs`` records ``(q, k_img, workspace)`` of every call."""

    def __init__(self):
        super().__init__()
        self.ptrs = []

    def daam_joint_tap_abi_version(self):
        return 1

    def daam_joint_tap_accumulate(self, q, kt, ki, dtype, batch, heads, P, T, Pk, d, qsb, qsh, qsp, tsb, tsh, tsp, isb, ish, isp, scale,
                                  weight, accumulate, sums, sums_stride_h, ws, ws_bytes, stream):
        rc = super().daam_joint_tap_accumulate(q, kt, ki, dtype, batch, heads, P, T, Pk, d, qsb, qsh, qsp, tsb, tsh, tsp, isb, ish, isp,
                                               scale, weight, accumulate, sums, sums_stride_h, ws, ws_bytes, stream)
        self.ptrs.append((int(q), int(ki or 0), int(ws)))
        qa, ta, ia = (_gather(p, dtype, batch, heads, rows, d, *st) for p, rows, st in
                      ((q, P, (qsb, qsh, qsp)), (kt, T, (tsb, tsh, tsp)), (ki, Pk, (isb, ish, isp))))
        p_pad = -(-P // TILE) * TILE
        mem = S._array(ws, ctypes.c_float, 2 * batch * heads * p_pad).reshape(batch * heads, p_pad, 2)
        c = F32(F64(F32(scale)) * LOG2E)
        for s in range(batch * heads):
            qs = qa[s // heads, s % heads].astype(F64)
            negm, rinv = emulate_stats((qs @ ta[s // heads, s % heads].astype(F64).T).astype(F32),
                                       (qs @ ia[s // heads, s % heads].astype(F64).T).astype(F32), c)
            mem[s, :P, 0], mem[s, :P, 1] = negm, rinv
        return rc


class FakeJointAffinityLib:
    """The two entry points in numpy (the f32 emulation of the image kernel on the statistics it is GIVEN) on CPU tensors' memory,
    held to the header's limits; records every call as ``(q, k_img, stats, stats_bytes, dtype, batch, heads, P, Pk, d, strides, scale,
    weight, accumulate)``."""

    def __init__(self):
        self.calls = []

    def daam_joint_affinity_stats_bytes(self, batch, heads, P):
        ok = batch >= 1 and heads >= 1 and batch * heads <= 4096 and 1 <= P <= 16384
        return 8 * batch * heads * (-(-P // TILE) * TILE) if ok else 0

    def daam_joint_affinity_accumulate(self, q, ki, stats, stats_bytes, dtype, batch, heads, P, Pk, d, qsb, qsh, qsp, isb, ish, isp, scale,
                                       weight, accumulate, sums, stream):
        assert q and ki and stats and sums and dtype in (DAAM_F16, DAAM_BF16) and d in J.HEAD_DIMS
        assert 1 <= P <= 16384 and 1 <= Pk <= 16384 and stats_bytes >= self.daam_joint_affinity_stats_bytes(batch, heads, P) > 0
        assert all(s >= 0 and s % 8 == 0 for s in (qsb, qsh, qsp, isb, ish, isp)) and q % 16 == 0 and ki % 16 == 0 and stats % 8 == 0
        assert math.isfinite(scale) and scale > 0 and math.isfinite(weight)
        self.calls.append((int(q), int(ki), int(stats), int(stats_bytes), dtype, batch, heads, P, Pk, d, (qsb, qsh, qsp, isb, ish, isp),
                           float(F32(scale)), float(F32(weight)), int(accumulate)))
        qa, ia = _gather(q, dtype, batch, heads, P, d, qsb, qsh, qsp), _gather(ki, dtype, batch, heads, Pk, d, isb, ish, isp)
        p_pad = -(-P // TILE) * TILE
        st = S._array(stats, ctypes.c_float, 2 * batch * heads * p_pad).reshape(batch * heads, p_pad, 2).copy()
        c = F32(F64(F32(scale)) * LOG2E)
        acc = np.zeros((P, Pk), F32)
        for s in range(batch * heads):
            raw_i = (qa[s // heads, s % heads].astype(F64) @ ia[s // heads, s % heads].astype(F64).T).astype(F32)
            acc = image_columns(raw_i, c, st[s, :P, 0], st[s, :P, 1], acc)
        out = S._array(sums, ctypes.c_float, P * Pk).reshape(P, Pk)
        out[:] = fma32(F32(weight), acc, out.copy() if accumulate else F32(0))
        return 0


def install(setattr_):
    """``_joint_domain.install`` with a joint library that leaves its statistics, plus a ``FakeJointAffinityLib`` under
    ``daam_amd.engine``; ``loads`` counts the calls of ``load_joint_affinity``.  Returns ``(engine module, joint lib, affinity lib,
    loads)``."""
    E, _ = J.install(setattr_)
    joint, aff, loads = FakeJointLibWithStats(), FakeJointAffinityLib(), []
    setattr_(E.nat, 'load_joint', lambda: joint)

    def load():
        loads.append(1)
        return aff
    setattr_(E.nat, 'load_joint_affinity', load)
    setattr_(E, '_joint_affinity_checked', False)
    return E, joint, aff, loads


# ---- the block-structured case: 3.22's construction carried to joint attention --------------------------------------------------------
BLOCK_GRID = (12, 20)
BLOCK_TEXT = 4
BLOCK_SEED = 0


def block_case(seed=BLOCK_SEED, d=64, dtype='f16'):
    """``(q = k_img f32 [1, 1, P, d], k_txt f32 [1, 1, 4, d], truth bool [12, 20], plane f32 [12, 20])``: a two-valued feature per cell
    (an ellipse and its ground) plus noise, so that the image block of the joint softmax is block-structured, a few text keys that
    take their share of every row, and a word map that is a Gaussian shifted off the ellipse."""
    h, w = BLOCK_GRID
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    truth = ((yy - 6) / 3.6) ** 2 + ((xx - 10.5) / 6.2) ** 2 <= 1.0
    a, b = rng.standard_normal(d), rng.standard_normal(d)
    feat = np.where(truth.reshape(-1, 1), a[None], b[None]) * 1.2 + 0.3 * rng.standard_normal((h * w, d))
    text = 1.2 * np.stack([a, b] * (BLOCK_TEXT // 2)) + 0.3 * rng.standard_normal((BLOCK_TEXT, d))      # two text keys per kind of cell
    plane = np.exp(-(((yy - 4) / 3.0) ** 2 + ((xx - 7.5) / 5.0) ** 2) / 2)
    return J.quantize(feat[None, None], dtype), J.quantize(text[None, None], dtype), truth, plane.astype(F32)


def propagate64(sums, m, iterations):
    """float64: ``iterations`` rounds of m <- (sums / rowsum) m on maps [N, P]."""
    s, m = np.asarray(sums, F64), np.asarray(m, F64)
    r = s.sum(axis=1)
    for _ in range(iterations):
        m = np.where(r == 0, m, (m @ s.T) / np.where(r == 0, 1, r))
    return m


def iou(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    return (a & b).sum() / max((a | b).sum(), 1)
