"""Shared by ``test_joint_tap_cpu.py`` and ``test_gpu_joint_tap.py``: the joint-attention tap (include/daam_joint_tap.h)
as a float64 numpy reference, a float32 emulation in the kernels' operation order (with the mutants that show the bound can fail),
the error bound, the inputs of the cases, and a numpy stand-in of ``libdaam_joint`` that puts the Python layer under test without a
GPU.  Test-only: the product has no fallback.

Inputs are f32 arrays q [batch, heads, P, d], k_txt [batch, heads, T, d], k_img [batch, heads, Pk, d] whose values are exactly
representable in the call's dtype ('f16' or 'bf16').  A call is ``(q, k_txt, k_img, scale, weight)``.  Planes are [T, P]
(``per_head``: [heads, T, P]).

The error bound, ``sums_bound``: ABSOLUTE per entry of ``sums`` of a chain of calls against float64 on the same fp16 / bf16 inputs
(u = 2^-24, the unit roundoff of f32; derived from the operations of daam_joint_tap.hip, nothing tuned on device output).  It is
bound (a) of ``_self_affinity_domain`` with the row running over the n = T + Pk keys of the joint softmax:

  * a logit: the product of two fp16 or two bf16 values is exact in f32; an any-order f32 sum of d of them carries (d - 1) u A_ij,
    A_ij = scale sum_c |q_ic k_jc|.  The device forms the exponent (base 2) as fma(raw, c, -(m c)), c = f32(scale log2 e): the
    rounding of c moves the argument by u |x_ij|, the fma's own rounding by u |x_ij - max_j x_ij|; the shift -(m c) is the SAME f32
    number in the statistics and in the text kernel (it is read back from the workspace), and a softmax does not change under a
    common shift, so its rounding cancels.  With |x_ij| <= A_ij:  theta_ij = (d + 1) u A_ij + u |x_ij - max_j x_ij|.  v_exp_f32 is
    within 1 ulp = 2 u:  tau_ij = theta_ij + 2 u.
  * the row sum l_i over all n keys: an any-order sum of n positive terms, (n - 1) u.  The online walk takes the text keys and then
    the image keys in steps of 32, and a step that holds no key at all (past the end of either kind) is skipped: there are
    steps = ceil(T / 32) + ceil(Pk / 32) of them.  Each rescales the running sum once, by exp2 of a rounded difference D <= 0
    (relative error of the carried part at most u |D| ln 2 + 2 u, weighted by 2^D <= 1: at most 3 u) plus a product and a sum (2 u):
    5 u per step.  Padded keys of a partial step enter as exp2(-inf) = 0 exactly.  The combination of the two lane halves (two
    exp2, two products, a sum) and the reciprocal: 10 u with slack.  c_row = (n - 1) + 5 steps + 10.
  * a softmax's first-order response to relative errors of its terms:

        |p_ij(device) - p_ij| <= p_ij (tau_ij + sum_l p_il tau_il + c_row u) (1 + 2^-9)  +  2^-126

    with the sum over l over ALL n keys (the floor: where exp2 leaves the normal range the device returns 0; (1 + 2^-9) covers
    exp(t) - 1 <= t (1 + t) for t < 2^-9).
  * a plane adds its S_plane slices (batch heads of them, or batch with a plane per head) with one fma each: S_plane u acc in all;
    the call ends with fma(weight, acc, previous): |weight| times the above plus u |result|.  A chain of calls adds its calls' bounds.
"""
import ctypes
import math

import numpy as np
import torch

import _sweep_domain as S
from _self_affinity_domain import U, bits, fma32, quantize  # noqa: F401  (bits, quantize: used by the tests)

F32, F64 = np.float32, np.float64
ROWS, KEY_TILE = 128, 64                    # query rows of a statistics block / cells of an output tile; keys per step, text rows of a tile
HEAD_DIMS = (64, 128)
LOG2E = 1.4426950408889634
DAAM_F16, DAAM_BF16 = 0, 2
E_INVALID = -1
REGIMES = ('small', 'peaked', 'outlier', 'zero_q')


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def inputs(regime, batch, heads, P, T, Pk, d, dtype, seed=0):
    """``(q, k_txt, k_img, scale)``: small logits; logits of about +-60 (image key i and text key t with (3 t + 1) mod P == i match
    query i: a peaked softmax that text and image share); one outlier image key (a text key where Pk == 0); an all-zero Q."""
    rng = np.random.default_rng(seed * 7919 + P * 31 + T * 17 + d)
    q = rng.standard_normal((batch, heads, P, d))
    kt = rng.standard_normal((batch, heads, T, d))
    ki = rng.standard_normal((batch, heads, Pk, d))
    scale = d ** -0.5
    if regime == 'peaked':
        g = (60.0 / math.sqrt(d)) ** 0.5
        ki = g * (q[:, :, np.arange(Pk) % P] + 0.1 * ki)
        kt = g * (q[:, :, (3 * np.arange(T) + 1) % P] + 0.1 * kt)
        q = g * q
    elif regime == 'outlier':
        q, kt, ki = 0.5 * q, 0.5 * kt, 0.5 * ki
        spike = 4.0 * np.sign(q.mean(axis=2))
        if Pk:
            ki[:, :, Pk // 2] = spike
        else:
            kt[:, :, T // 2] = spike
    elif regime == 'zero_q':
        q = np.zeros_like(q)
    else:
        q, kt, ki = 0.5 * q, 0.5 * kt, 0.5 * ki
    return quantize(q, dtype), quantize(kt, dtype), quantize(ki, dtype), float(F32(scale))


PS = (1, 5, 63, 65, 130, 257)
TS = (1, 7, 64, 77, 154, 333)
SLICES = ((1, 1), (1, 3), (2, 3))                     # (batch, heads)
LAYOUTS = ('interleaved', 'packed')


def _case(P, T, Pk, d, dtype, i, di, ti, fam):
    return (P, T, Pk, d, dtype, SLICES[(i + di + ti + fam) % 3], LAYOUTS[(i + di + ti // 1 + fam // 2) % 2], bool((i + di + ti + fam) % 2),
            REGIMES[(i + di + 2 * ti + fam) % 4])


# (P, T, Pk, d, dtype, (batch, heads), layout, per_head, regime).  Three families of 24: every P x head dim x dtype (twice, with
# other partners) and every T x head dim x dtype; the partner sizes, slice counts, layouts, output modes and regimes rotate so that
# each value meets every head dim and both dtypes.  Then Pk = 0 (the text-only softmax) and Pk = 200 != P = 65, once per head dim.
CASES = [_case(P, TS[(pi + 2 * di + 3 * ti) % 6], P, d, dtype, pi, di, ti, 0)
         for pi, P in enumerate(PS) for di, d in enumerate(HEAD_DIMS) for ti, dtype in enumerate(('f16', 'bf16'))]
CASES += [_case(PS[(xi + 3 + di + 2 * ti) % 6], T, PS[(xi + 3 + di + 2 * ti) % 6], d, dtype, xi, di, ti, 1)
          for xi, T in enumerate(TS) for di, d in enumerate(HEAD_DIMS) for ti, dtype in enumerate(('f16', 'bf16'))]
CASES += [_case(P, TS[(pi + 1 + di + 2 * ti) % 6], P, d, dtype, pi, di, ti, 2)
          for pi, P in enumerate(PS) for di, d in enumerate(HEAD_DIMS) for ti, dtype in enumerate(('f16', 'bf16'))]
CASES += [(65, 77, 0, 64, 'f16', (2, 3), 'interleaved', False, 'small'), (130, 154, 0, 128, 'bf16', (1, 3), 'packed', True, 'peaked'),
          (65, 77, 200, 64, 'bf16', (1, 3), 'packed', True, 'outlier'), (65, 154, 200, 128, 'f16', (2, 3), 'interleaved', False, 'small')]
CASES = list(dict.fromkeys(CASES))


def case_id(c):
    return f'P{c[0]}-T{c[1]}-Pk{c[2]}-d{c[3]}-{c[4]}-S{c[5][0]}x{c[5][1]}-{c[6]}-{"heads" if c[7] else "one"}-{c[8]}'


def case_inputs(c):
    P, T, Pk, d, dtype, (batch, heads) = c[:6]
    return inputs(c[8], batch, heads, P, T, Pk, d, dtype, seed=P + T + d)


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------
def logits64(q, kt, ki, scale):
    """float64 [b, h, P, T + Pk]: text columns first."""
    k = np.concatenate([kt, ki], axis=2).astype(F64)
    return float(F32(scale)) * np.einsum('bhic,bhjc->bhij', q.astype(F64), k)


def softmax64(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _planes(p_txt, per_head):
    """[b, h, P, T] -> [T, P] (the sum over slices) or [h, T, P] (over the batch)."""
    return p_txt.sum(axis=0).transpose(0, 2, 1) if per_head else p_txt.sum(axis=(0, 1)).T


def image_share(q, kt, ki, scale):
    """The least, over rows, of the probability mass on the image keys."""
    return float(softmax64(logits64(q, kt, ki, scale))[..., kt.shape[2]:].sum(axis=-1).min())


def reference_sums(calls, per_head=False, prior=None):
    """float64 planes: the first call overwrites (``accumulate == 0``) unless ``prior`` is given."""
    out = None if prior is None else np.asarray(prior, F64)
    for q, kt, ki, scale, weight in calls:
        acc = _planes(softmax64(logits64(q, kt, ki, scale))[..., :kt.shape[2]], per_head)
        out = float(F32(weight)) * acc + (0.0 if out is None else out)
    return out


def reference_text_only(q, kt, scale):
    """float64 [T, P]: the UNet's softmax over the text keys alone, summed over slices."""
    x = float(F32(scale)) * np.einsum('bhic,bhjc->bhij', q.astype(F64), kt.astype(F64))
    return softmax64(x).sum(axis=(0, 1)).T


# ---- bound (module docstring) --------------------------------------------------------------------------------------------------------
def sums_bound(calls, per_head=False, prior_bound=None, prior=None):
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
        acc = _planes(p[..., :T], per_head)
        s_plane = b if per_head else b * h
        value = float(F32(weight)) * acc + (0.0 if value is None else value)
        bound = bound + w * (_planes(per[..., :T], per_head) + s_plane * U * acc) + U * np.abs(value) * (1 + 2.0 ** -9)
    return bound


# ---- float32 emulation ---------------------------------------------------------------------------------------------------------------
def _acc_rows(half):
    return [(reg & 3) + 8 * (reg >> 2) + 4 * half for reg in range(16)]


def emulate_stats(raw_t, raw_i, c, count_padded=False):
    """``(negm, rinv)`` f32 [P] of one slice's raw dot products f32 [P, T] and [P, Pk]: the maximum over all keys, then per lane half
    the 16-term partial sums of every 32-key step in register order, the text steps and then the image steps added ascending, the
    lower half first.  (The device rescales a running sum where this uses the final maximum: the bound covers either.)"""
    P = raw_t.shape[0]
    negm = -(np.concatenate([raw_t, raw_i], axis=1).max(axis=1) * c).astype(F32)
    halves = [np.zeros(P, F32), np.zeros(P, F32)]
    for raw in (raw_t, raw_i):
        n = raw.shape[1]
        pad = -(-n // 32) * 32
        y = np.full((P, pad), -np.inf, F32)
        y[:, :n] = fma32(raw, c, negm[:, None])
        if count_padded:
            y[:, n:] = negm[:, None]                 # a zero-filled key: raw = 0
        e = np.exp2(y).astype(F32).reshape(P, pad // 32, 32)
        for t in range(pad // 32):
            for half in (0, 1):
                part = np.zeros(P, F32)
                for row in _acc_rows(half):
                    part = part + e[:, t, row]
                halves[half] = halves[half] + part
    return negm, (F32(1) / (halves[0] + halves[1])).astype(F32)


MUTANTS = ('no_image_keys', 'no_scale', 'padded_keys', 'neighbour_stats', 'packed_head_stride', 'all_to_plane0')


def emulate_sums(calls, per_head=False, prior=None, mutant=None):
    """f32 planes in the order of the two kernels.  ``mutant``: one of ``MUTANTS``."""
    out = None if prior is None else np.asarray(prior, F32)
    for q, kt, ki, scale, weight in calls:
        b, h, P, d = q.shape
        T = kt.shape[2]
        c = F32(LOG2E if mutant == 'no_scale' else F64(F32(scale)) * LOG2E)
        if mutant == 'packed_head_stride':            # [b, rows, h d] memory read as if it were [b, h, rows, d]
            q, kt, ki = (x.transpose(0, 2, 1, 3).reshape(x.shape) for x in (q, kt, ki))
        acc = np.zeros((h, T, P) if per_head else (T, P), F32)
        for s in range(b * h):
            qs = q[s // h, s % h].astype(F64)
            raw_t = (qs @ kt[s // h, s % h].astype(F64).T).astype(F32)
            raw_i = (qs @ ki[s // h, s % h].astype(F64).T).astype(F32)
            negm, rinv = emulate_stats(raw_t, raw_i[:, :0] if mutant == 'no_image_keys' else raw_i, c, count_padded=mutant == 'padded_keys')
            if mutant == 'neighbour_stats':
                negm, rinv = np.roll(negm, -1), np.roll(rinv, -1)
            plane = acc[0 if mutant == 'all_to_plane0' else s % h] if per_head else acc
            plane[...] = fma32(np.exp2(fma32(raw_t, c, negm[:, None])).astype(F32), rinv[:, None], plane.T).T
        out = fma32(F32(weight), acc, F32(0) if out is None else out)
    return out


# ---- a numpy stand-in of libdaam_joint -----------------------------------------------------------------------------------------------
class FakeJointLib:
    """The two entry points in numpy (the f32 emulation) on CPU tensors' memory, held to the header's limits; records every call as
    ``(dtype, batch, heads, P, T, Pk, d, strides, scale, weight, accumulate, sums_stride_h)``."""

    def __init__(self):
        self.calls = []

    def daam_joint_tap_workspace(self, batch, heads, P):
        ok = batch >= 1 and heads >= 1 and batch * heads <= 4096 and 1 <= P <= 16384
        return 8 * batch * heads * (-(-P // ROWS) * ROWS) if ok else 0

    def daam_joint_tap_accumulate(self, q, kt, ki, dtype, batch, heads, P, T, Pk, d, qsb, qsh, qsp, tsb, tsh, tsp, isb, ish, isp, scale,
                                  weight, accumulate, sums, sums_stride_h, ws, ws_bytes, stream):
        assert q and kt and (ki or not Pk) and sums and ws and dtype in (DAAM_F16, DAAM_BF16) and d in HEAD_DIMS
        assert 1 <= P <= 16384 and 1 <= T <= 512 and 0 <= Pk <= 16384
        assert ws_bytes >= self.daam_joint_tap_workspace(batch, heads, P) > 0
        assert all(s >= 0 and s % 8 == 0 for s in (qsb, qsh, qsp, tsb, tsh, tsp, isb, ish, isp)) and q % 16 == 0 and kt % 16 == 0
        assert math.isfinite(scale) and scale > 0 and math.isfinite(weight) and (sums_stride_h == 0 or sums_stride_h >= T * P)
        self.calls.append((dtype, batch, heads, P, T, Pk, d, (qsb, qsh, qsp, tsb, tsh, tsp, isb, ish, isp), float(F32(scale)),
                           float(F32(weight)), int(accumulate), int(sums_stride_h)))

        def gather(ptr, rows, sb, sh, sp):
            if not rows:
                return np.zeros((batch, heads, 0, d), F32)
            n = (batch - 1) * sb + (heads - 1) * sh + (rows - 1) * sp + d
            raw = torch.from_numpy(S._array(ptr, ctypes.c_int16, n).copy())
            vals = raw.view(torch.float16 if dtype == DAAM_F16 else torch.bfloat16).float().numpy()
            return np.lib.stride_tricks.as_strided(vals, (batch, heads, rows, d), tuple(4 * s for s in (sb, sh, sp, 1))).copy()
        per_head = sums_stride_h != 0
        planes = heads if per_head else 1
        stride = sums_stride_h if per_head else T * P
        mem = S._array(sums, ctypes.c_float, (planes - 1) * stride + T * P)
        view = np.lib.stride_tricks.as_strided(mem, (planes, T, P), (4 * stride, 4 * P, 4))
        prior = (view.copy() if per_head else view[0].copy()) if accumulate else None
        got = emulate_sums([(gather(q, P, qsb, qsh, qsp), gather(kt, T, tsb, tsh, tsp), gather(ki, Pk, isb, ish, isp), scale, weight)],
                           per_head=per_head, prior=prior)
        view[...] = got if per_head else got[None]
        return 0


def install(setattr_):
    """``_sweep_domain.install`` (CPU tensors pass for device tensors) plus a ``FakeJointLib`` under ``daam_amd.engine``.
    Returns ``(engine module, lib)``."""
    E, _ = S.install(setattr_)
    lib = FakeJointLib()
    setattr_(E.nat, 'load_joint', lambda: lib)
    setattr_(E, '_check_on_device', lambda query, key: None)
    return E, lib
