"""Shared by ``test_joint_attend_cpu.py`` and ``test_gpu_joint_attend.py``: the fused joint attention (include/daam_joint_attend.h,
DESIGN 3.28) as a float64 numpy reference, a float32 emulation in the kernel's operation order (with the mutants that show the bound
can fail), the error bound, the inputs of the cases, and a recording stand-in of ``libdaam_jointattend`` that puts the Python layer
under test without a GPU.  Test-only: the product has no fallback.

Inputs are a dict of f32 arrays ``qi, ki, vi`` [batch, heads, P, d] and ``qt, kt, vt`` [batch, heads, T, d] whose values are exactly
representable in the call's dtype ('f16' or 'bf16'), plus ``scale``.  Keys are walked text first, then image: key j of the walk.

The error bound of an output element, ``out_bound``: ABSOLUTE against float64 on the same inputs (u = 2^-24; u16 = 2^-11 for fp16,
2^-8 for bf16; derived from the operations of daam_joint_attend.hip, nothing tuned on device output).  The device computes
o_ic = rnd16((sum_j e~_ij v_jc, rescaled) (1 / l_i)) with e~ the exponential relative to the running maximum, rounded to the dtype:

  * e_ij K_i / l_i against p_ij: bound (a) of 3.22 / 3.24 (``_joint_domain``): p_ij (tau_ij + sum_l p_il tau_il + c_row u) (1 + 2^-9)
    + 2^-126, tau_ij = (d + 1) u A_ij + u |x_ij - max x_i.| + 2 u, c_row = (n - 1) + 5 steps + 10, steps = ceil(T / 32) + ceil(P / 32)
    the 32-key steps of this kernel's walk (the same count as the tap's walk over the same keys).
  * the rounding of e~ to the dtype: relative u16; below the dtype's normal range (fp16: e < 2^-14) absolute 2^-25, which the later
    factors (rescales <= 1, 1 / l <= 1 since the maximum's own term is 1) do not enlarge: a floor of 2^-25 per key.  bf16: the
    fragment carries 2^-15 e (an exact product), so that sum e v stays inside f32 for any bf16 V; it leaves the normal range where
    e < 2^-111: a floor of 2^-111 per key.
  * the output accumulator: an any-order f32 sum over n keys, n u; it is multiplied by exp2 of the maximum's move once per step,
    each such factor within 3 u (as for l in 3.24; where the maximum stays the factor is exactly 1): 3 steps u.
  * the product with 1 / l: u.  Together, per key, p_ij eps_ij |v_jc| with
    eps_ij = (a)_ij / p_ij + u16 + (n + 3 steps + 1) u, summed with |v|: cancelling V is covered.
  * the one rounding of the result: u16 (|o_ic| + the above), or absolutely 2^-25 where an fp16 result is subnormal (bf16: 2^-126).

The statistics are held through the probabilities they define, p^_ij = 2^(raw_ij c + stats.x) stats.y for ALL keys, to bound (a)
unchanged; the text planes formed from them to ``_joint_domain.sums_bound`` unchanged.
"""
import ctypes
import math

import numpy as np

import _joint_domain as J
import _sweep_domain as S
from _joint_domain import F32, F64, LOG2E, U, bits, fma32, quantize  # noqa: F401

DAAM_F16, DAAM_BF16 = J.DAAM_F16, J.DAAM_BF16
E_INVALID = -1
U16 = {'f16': 2.0 ** -11, 'bf16': 2.0 ** -8}
SUB16 = {'f16': (2.0 ** -14, 2.0 ** -25), 'bf16': (2.0 ** -111, 2.0 ** -111)}     # (least e rounded relatively, absolute error below it)
HUGE16 = {'f16': 65504.0, 'bf16': 3.3895313892515355e38}                         # the largest finite values
FOLD = {'f16': 1.0, 'bf16': 2.0 ** -15}                                            # the factor the fragment of e carries (Round16)
LOGITS = ('small', 'late_outlier', 'peaked', 'zero_q', 'rising')
VALUES = ('normal', 'ramp', 'cancel', 'huge', 'subnormal')


def pad128(P):
    return -(-P // 128) * 128


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def inputs(logits, values, batch, heads, P, T, d, dtype, seed=0):
    """Logit regimes: small; one outlier image key placed LATE in the walk (the last but one); about +-60 peaked (query i of either
    kind matches image key i mod P and text key t with (3 t + 1) mod P == i mod P); all-zero Q; logits RISING along the walk, so the
    running maximum moves in every step.  V regimes: unit normal; v[j][c] = (j + 1) (1 + c mod 4) / 256, distinct per key of the walk;
    alternating signs that cancel; magnitudes in [0.25, 0.9] of the dtype's largest finite value (a convex combination formed with
    weights rounded up by u16 stays finite below 1 / (1 + 2 u16) of it); fp16 subnormals
    (multiples of 2^-24 below 2^-14)."""
    rng = np.random.default_rng(seed * 7919 + P * 31 + T * 17 + d)
    n = T + P
    q = rng.standard_normal((batch, heads, n, d))         # rows 0 .. T - 1 the text queries, then the image queries: the walk's order
    k = rng.standard_normal((batch, heads, n, d))
    scale = d ** -0.5
    if logits == 'peaked':
        g = (60.0 / math.sqrt(d)) ** 0.5
        target = np.concatenate([(3 * np.arange(T) + 1) % P, np.arange(P)]) + T          # the image query a key matches
        k = g * (q[:, :, target] + 0.1 * k)
        q[:, :, :T] = q[:, :, T + np.arange(T) % P]                                        # text query t looks like image query t mod P
        q = g * q
    elif logits == 'late_outlier':
        q, k = 0.5 * q, 0.5 * k
        k[:, :, n - 2 if P > 1 else n - 1] = 4.0 * np.sign(q.mean(axis=2))
    elif logits == 'zero_q':
        q = np.zeros_like(q)
    elif logits == 'rising':
        u = np.sign(rng.standard_normal(d)) / math.sqrt(d)
        q = 4.0 * math.sqrt(d) ** 0.5 * u + 0.05 * q
        k = (3.0 * math.sqrt(d) ** 0.5 * (np.arange(n)[:, None] + 1) / n) * u + 0.05 * k   # x_ij about 12 (j + 1) / n
    else:
        q, k = 0.5 * q, 0.5 * k
    j = np.arange(n)[:, None]
    c = np.arange(d)[None, :]
    if values == 'ramp':
        v = np.broadcast_to((j + 1) * (1 + c % 4) / 256.0, (batch, heads, n, d)).copy()
    elif values == 'cancel':
        v = np.where(j % 2 == 0, 1.0, -1.0) * (1.0 + 2.0 ** -6 * rng.integers(0, 4, (batch, heads, n, d)))
    elif values == 'huge':
        v = HUGE16[dtype] * rng.uniform(0.25, 0.9, (batch, heads, n, d)) * np.sign(rng.standard_normal((batch, heads, n, d)))
    elif values == 'subnormal':
        v = 2.0 ** -24 * rng.integers(-1023, 1024, (batch, heads, n, d))
    else:
        v = rng.standard_normal((batch, heads, n, d))
    qz = lambda x: quantize(x, dtype)
    return dict(qt=qz(q[:, :, :T]), qi=qz(q[:, :, T:]), kt=qz(k[:, :, :T]), ki=qz(k[:, :, T:]), vt=qz(v[:, :, :T]), vi=qz(v[:, :, T:]),
                scale=float(F32(scale)), dtype=dtype)


PS = (1, 5, 63, 65, 130, 257)
TS = (1, 7, 64, 77, 154, 333)

# (P, T, d, dtype, (batch, heads), layout, logits, values): every P x head dim x dtype; T, slice counts, layouts and regimes rotate.
CASES = [(P, TS[(pi + 2 * di + 3 * ti) % 6], d, dtype, J.SLICES[(pi + di + ti) % 3], J.LAYOUTS[(pi + di) % 2],
          LOGITS[(pi + 2 * di + 3 * ti) % 5], VALUES[(pi + di + 2 * ti) % 5])
         for pi, P in enumerate(PS) for di, d in enumerate(J.HEAD_DIMS) for ti, dtype in enumerate(('f16', 'bf16'))]
# the pairs the rotation above leaves out and the issue names: rising logits against per-key V at every head dim and dtype, the late
# outlier against cancelling V, peaked logits against the largest V
CASES += [(65, 77, 64, 'f16', (1, 3), 'interleaved', 'rising', 'ramp'), (130, 154, 128, 'bf16', (1, 3), 'packed', 'rising', 'ramp'),
          (257, 333, 64, 'bf16', (1, 1), 'packed', 'rising', 'ramp'), (63, 64, 128, 'f16', (2, 3), 'interleaved', 'rising', 'ramp'),
          (130, 77, 64, 'f16', (1, 3), 'packed', 'late_outlier', 'cancel'), (65, 7, 128, 'bf16', (2, 3), 'interleaved', 'peaked', 'huge'),
          (5, 1, 64, 'f16', (1, 1), 'packed', 'small', 'subnormal')]
CASES = list(dict.fromkeys(CASES))


def case_id(c):
    return f'P{c[0]}-T{c[1]}-d{c[2]}-{c[3]}-S{c[4][0]}x{c[4][1]}-{c[5]}-{c[6]}-{c[7]}'


def case_inputs(c):
    P, T, d, dtype, (batch, heads), _, logits, values = c
    return inputs(logits, values, batch, heads, P, T, d, dtype, seed=P + T + d)


# ---- float64 reference ---------------------------------------------------------------------------------------------------------------
def _cat(inp, name):
    return np.concatenate([inp[name + 't'], inp[name + 'i']], axis=2).astype(F64)


def reference(inp):
    """``(out_img [b, h, P, d], out_txt [b, h, T, d], p [b, h, T + P, T + P])`` in float64; query rows in the walk's order."""
    T = inp['kt'].shape[2]
    x = inp['scale'] * np.einsum('bhic,bhjc->bhij', _cat(inp, 'q'), _cat(inp, 'k'))
    p = J.softmax64(x)
    o = np.einsum('bhij,bhjc->bhic', p, _cat(inp, 'v'))
    return o[:, :, T:], o[:, :, :T], p


def _per_probability(inp):
    """Bound (a) of every probability, [b, h, T + P, T + P], and the probabilities."""
    d, T, n = inp['qi'].shape[3], inp['kt'].shape[2], inp['kt'].shape[2] + inp['ki'].shape[2]
    x = inp['scale'] * np.einsum('bhic,bhjc->bhij', _cat(inp, 'q'), _cat(inp, 'k'))
    a = inp['scale'] * np.einsum('bhic,bhjc->bhij', np.abs(_cat(inp, 'q')), np.abs(_cat(inp, 'k')))
    p = J.softmax64(x)
    tau = (d + 1) * U * a + U * np.abs(x - x.max(axis=-1, keepdims=True)) + 2 * U
    steps = -(-T // 32) + -(-(n - T) // 32)
    c_row = (n - 1) + 5 * steps + 10
    return p * (tau + (p * tau).sum(axis=-1, keepdims=True) + c_row * U) * (1 + 2.0 ** -9) + 2.0 ** -126, p, steps


def out_bound(inp):
    """``(bound_img, bound_txt)`` of the outputs (module docstring)."""
    T, n, dtype = inp['kt'].shape[2], inp['kt'].shape[2] + inp['ki'].shape[2], inp['dtype']
    per, p, steps = _per_probability(inp)
    v = np.abs(_cat(inp, 'v'))
    u16, (_, floor16) = U16[dtype], SUB16[dtype]
    weight = per + p * (u16 + (n + 3 * steps + 1) * U) * (1 + 2.0 ** -9) + floor16
    before = np.einsum('bhij,bhjc->bhic', weight, v)
    o = np.abs(np.einsum('bhij,bhjc->bhic', p, _cat(inp, 'v')))
    bound = before + u16 * (o + before) + (floor16 if dtype == 'f16' else 2.0 ** -126)
    return bound[:, :, T:], bound[:, :, :T]


def stats_probabilities(inp, stats):
    """float64 [b, h, P, T + P]: what ``stats`` f32 [b h, pad128(P), 2] make of the exact raw dot products of the image queries."""
    b, h, P, _ = inp['qi'].shape
    raw = np.einsum('bhic,bhjc->bhij', inp['qi'].astype(F64), _cat(inp, 'k'))
    c = float(F32(F64(F32(inp['scale'])) * LOG2E))
    st = stats.reshape(b, h, -1, 2)[:, :, :P].astype(F64)
    with np.errstate(over='ignore'):
        return np.exp2(raw * c + st[..., 0:1]) * st[..., 1:2]


def stats_bound(inp):
    """Bound (a) of the image rows, [b, h, P, T + P], and the float64 probabilities."""
    T = inp['kt'].shape[2]
    per, p, _ = _per_probability(inp)
    return per[:, :, T:], p[:, :, T:]


def tap_calls(inp, first=0, weight=1.0):
    """The call of ``_joint_domain`` (``reference_sums`` / ``sums_bound``) that the text planes of batch entries ``first ..`` are."""
    return [(inp['qi'][first:], inp['kt'][first:], inp['ki'][first:], inp['scale'], weight)]


# ---- float32 emulation ---------------------------------------------------------------------------------------------------------------
MUTANTS = ('v_natural_order', 'no_rescale', 'no_text_in_l', 'no_divide', 'padded_keys', 'text_rows_image_stats', 'packed_head_stride',
           'neighbour_stats')
_HALF_ROWS = [[(reg & 3) + 8 * (reg >> 2) + 4 * half for reg in range(16)] for half in (0, 1)]
# element j of lane half h of the P fragment of a 16-key k-step is key 8 (j >> 2) + 4 h + (j & 3); a V fragment in natural order has
# key 8 h + j there
_P_KEY = np.array([8 * (j >> 2) + 4 * h + (j & 3) for h in (0, 1) for j in range(8)])
_V_NATURAL = np.array([8 * h + j for h in (0, 1) for j in range(8)])


def shows(mutant, case):
    """Whether ``mutant`` can show on ``case``: the others are bit-equal or inside the bound by construction."""
    P, T, d, dtype, (batch, heads), layout, logits, values = case
    plain_v = values in ('normal', 'ramp', 'huge')        # cancelling or tiny V: the bound's sum of |p v| dwarfs what a mutant moves
    if mutant == 'v_natural_order':                       # equal weights inside a k-step, or V rising as slowly as the weights, hide it
        return logits in ('small', 'late_outlier', 'peaked') and plain_v and P >= 5
    if mutant == 'no_rescale':                            # the maximum has to move after a step that carries weight
        return logits in ('rising', 'late_outlier') and T + P > 64
    if mutant == 'padded_keys':                           # against bf16's u16 a few zero keys among hundreds stay inside
        return (T % 32 != 0 or P % 32 != 0) and logits in ('small', 'zero_q') and plain_v and (dtype == 'f16' or T + P < 64)
    if mutant == 'text_rows_image_stats':                 # rows whose sums l differ
        return logits in ('small', 'late_outlier') and plain_v and P > 1
    if mutant == 'packed_head_stride':
        return heads > 1 and layout == 'interleaved' and logits != 'zero_q' and plain_v and P > 1
    if mutant == 'no_divide':
        return plain_v
    if mutant == 'no_text_in_l':
        return plain_v and logits in ('small', 'zero_q')
    return True


def _walk(raw, v, c, dtype, limits, mutant=None):
    """One slice, the query rows of ``raw`` f32 [R, T + P] (text columns first, ``limits`` = (T, P)) against ``v`` f32 [T + P, d]:
    ``(acc [R, d], negm [R], l [R])`` in f32 in the order of the kernel -- steps of 32 keys per kind, the maximum shared by the lane
    halves, l per half, the accumulator rescaled and fed e rounded to the dtype in k-steps of 16."""
    R, d = raw.shape[0], v.shape[1]
    acc = np.zeros((R, d), F32)
    m = np.full(R, -np.inf, F32)
    negm = np.zeros(R, F32)
    halves = [np.zeros(R, F32), np.zeros(R, F32)]
    base = 0
    for kind, n in enumerate(limits):
        for k0 in range(0, n, 32):
            x = np.full((R, 32), -np.inf, F32)
            vv = np.zeros((32, d), F32)
            w = min(32, n - k0)
            x[:, :w] = raw[:, base + k0:base + k0 + w]
            vv[:w] = v[base + k0:base + k0 + w]
            if mutant == 'padded_keys':
                x[:, w:] = 0
            m_new = np.maximum(m, x.max(axis=1))
            negm_new = (-(m_new * c)).astype(F32)
            with np.errstate(invalid='ignore', over='ignore'):
                carry = np.where(np.isfinite(m), np.exp2((negm_new - negm).astype(F32)), 0).astype(F32)
            e = np.exp2(fma32(x, c, negm_new[:, None])).astype(F32)
            count = not (mutant == 'no_text_in_l' and kind == 0)
            for half in (0, 1):
                part = np.zeros(R, F32)
                for row in _HALF_ROWS[half]:
                    part = part + e[:, row]
                halves[half] = (halves[half] * carry + (part if count else 0)).astype(F32)
            if mutant != 'no_rescale':
                acc = (acc * carry[:, None]).astype(F32)
            e16 = quantize(e * F32(FOLD[dtype]), dtype)
            for ks in (0, 1):
                pk = e16[:, 16 * ks + _P_KEY]
                vk = vv[16 * ks + (_V_NATURAL if mutant == 'v_natural_order' else _P_KEY)]
                acc = (acc + (pk.astype(F64) @ vk.astype(F64)).astype(F32)).astype(F32)
            m, negm = m_new, negm_new
        base += n
    return acc, negm, (halves[0] + halves[1]).astype(F32)


def emulate(inp, mutant=None):
    """``(out_img, out_txt, stats)``: outputs f32 holding dtype values, [b, h, rows, d]; stats f32 [b h, pad128(P), 2]."""
    b, h, P, d = inp['qi'].shape
    T, dtype = inp['kt'].shape[2], inp['dtype']
    c = F32(F64(F32(inp['scale'])) * LOG2E)
    src = dict(inp)
    if mutant == 'packed_head_stride':                    # [b, rows, h d] memory read as if it were [b, h, rows, d]
        for key in ('qi', 'ki', 'vi', 'qt', 'kt', 'vt'):
            src[key] = inp[key].transpose(0, 2, 1, 3).reshape(inp[key].shape)
    oi, ot = np.zeros((b, h, P, d), F32), np.zeros((b, h, T, d), F32)
    stats = np.zeros((b * h, pad128(P), 2), F32)
    for s in range(b * h):
        bi, hi = s // h, s % h
        k = np.concatenate([src['kt'][bi, hi], src['ki'][bi, hi]]).astype(F64)
        v = np.concatenate([src['vt'][bi, hi], src['vi'][bi, hi]])
        rinv_img = None
        for name, out in (('qi', oi), ('qt', ot)):
            raw = (src[name][bi, hi].astype(F64) @ k.T).astype(F32)
            acc, negm, l = _walk(raw, v, c, dtype, (T, P), mutant)
            rinv = (F32(1) / l).astype(F32)
            if name == 'qi':
                stats[s, :P, 0], stats[s, :P, 1] = negm, rinv
                rinv_img = rinv
            elif mutant == 'text_rows_image_stats':
                rinv = rinv_img[np.arange(T) % P]
            with np.errstate(over='ignore'):
                out[bi, hi] = quantize(acc if mutant == 'no_divide' else acc * (rinv * F32(1 / FOLD[dtype]))[:, None], dtype)
    return oi, ot, stats


def emulate_text(inp, stats, per_head=False, first=0, weight=1.0, prior=None, mutant=None):
    """The text kernel on given statistics f32 [b h, pad128(P), 2]: f32 planes [T, P] or [heads, T, P] of batch entries ``first ..``."""
    b, h, P, d = inp['qi'].shape
    T = inp['kt'].shape[2]
    c = F32(F64(F32(inp['scale'])) * LOG2E)
    acc = np.zeros((h, T, P) if per_head else (T, P), F32)
    for s in range(first * h, b * h):
        raw_t = (inp['qi'][s // h, s % h].astype(F64) @ inp['kt'][s // h, s % h].astype(F64).T).astype(F32)
        negm, rinv = stats[s, :P, 0], stats[s, :P, 1]
        if mutant == 'neighbour_stats':
            negm, rinv = np.roll(negm, -1), np.roll(rinv, -1)
        plane = acc[s % h] if per_head else acc
        plane[...] = fma32(np.exp2(fma32(raw_t, c, negm[:, None])).astype(F32), rinv[:, None], plane.T).T
    return fma32(F32(weight), acc, F32(0) if prior is None else np.asarray(prior, F32))


def worst(got, want, bound):
    """The largest error / bound."""
    return float((np.abs(np.asarray(got, F64) - want) / bound).max())


# ---- a recording stand-in of libdaam_jointattend ----------------------------------------------------------------------------------------
class FakeJointAttendLib:
    """Both entry points, held to the header's limits: ``forward`` fills its outputs with 0.25 and its statistics with (0, 1 / (T + P))
    -- those of an all-zero Q -- and ``text`` adds ``weight * slices / (T + P)``; every call is recorded as a dict of its arguments."""

    def __init__(self):
        self.forwards, self.texts = [], []

    def daam_joint_attend_abi_version(self):
        return 1

    def daam_joint_attend_stats_bytes(self, batch, heads, P):
        ok = batch >= 1 and heads >= 1 and batch * heads <= 4096 and 1 <= P <= 16384
        return 8 * batch * heads * pad128(P) if ok else 0

    def daam_joint_attend_forward(self, qi, ki, vi, qt, kt, vt, oi, ot, dtype, batch, heads, P, T, d, img_st, txt_st, out_st, scale, stats,
                                  stats_bytes, stream):
        img_st, txt_st, out_st = list(img_st), list(txt_st), list(out_st)
        assert all((qi, ki, vi, qt, kt, vt, oi, ot)) and dtype in (DAAM_F16, DAAM_BF16) and d in J.HEAD_DIMS
        assert 1 <= P <= 16384 and 1 <= T <= 512 and math.isfinite(scale) and scale > 0
        assert len(img_st) == 9 and len(txt_st) == 9 and len(out_st) == 6 and all(s >= 0 and s % 8 == 0 for s in img_st + txt_st + out_st)
        assert all(p % 16 == 0 for p in (qi, ki, vi, qt, kt, vt, oi, ot))
        assert stats is None or (stats % 8 == 0 and stats_bytes >= self.daam_joint_attend_stats_bytes(batch, heads, P) > 0)
        self.forwards.append(dict(ptrs=(qi, ki, vi, qt, kt, vt), outs=(oi, ot), dtype=dtype, batch=batch, heads=heads, P=P, T=T, d=d,
                                  strides=(img_st, txt_st, out_st), scale=float(F32(scale)), stats=stats, stats_bytes=stats_bytes))
        quarter = 0x3400 if dtype == DAAM_F16 else 0x3E80
        for ptr, rows, (sb, sh, sp) in ((oi, P, out_st[:3]), (ot, T, out_st[3:])):
            mem = S._array(ptr, ctypes.c_uint16, (batch - 1) * sb + (heads - 1) * sh + (rows - 1) * sp + d)
            view = np.lib.stride_tricks.as_strided(mem, (batch, heads, rows, d), (2 * sb, 2 * sh, 2 * sp, 2))
            view[...] = quarter
        if stats:
            st = S._array(stats, ctypes.c_float, 2 * batch * heads * pad128(P)).reshape(-1, 2)
            st[:, 0], st[:, 1] = 0, F32(1) / F32(T + P)
        return 0

    def daam_joint_attend_text(self, q, kt, stats, stats_bytes, dtype, batch, heads, P, T, d, qsb, qsh, qsp, tsb, tsh, tsp, scale, weight,
                               accumulate, sums, sums_stride_h, stream):
        assert q and kt and stats and sums and dtype in (DAAM_F16, DAAM_BF16) and d in J.HEAD_DIMS and stats % 8 == 0
        assert stats_bytes >= self.daam_joint_attend_stats_bytes(batch, heads, P) > 0
        assert all(s >= 0 and s % 8 == 0 for s in (qsb, qsh, qsp, tsb, tsh, tsp)) and q % 16 == 0 and kt % 16 == 0
        assert sums_stride_h == 0 or sums_stride_h >= T * P
        self.texts.append(dict(q=q, kt=kt, stats=stats, stats_bytes=stats_bytes, dtype=dtype, batch=batch, heads=heads, P=P, T=T, d=d,
                               strides=(qsb, qsh, qsp, tsb, tsh, tsp), scale=float(F32(scale)), weight=float(F32(weight)),
                               accumulate=int(accumulate), sums=sums, sums_stride_h=int(sums_stride_h)))
        st = S._array(stats, ctypes.c_float, 2 * batch * heads * pad128(P)).reshape(batch * heads, pad128(P), 2)
        planes = heads if sums_stride_h else 1
        stride = sums_stride_h or T * P
        mem = S._array(sums, ctypes.c_float, (planes - 1) * stride + T * P)
        view = np.lib.stride_tricks.as_strided(mem, (planes, T, P), (4 * stride, 4 * P, 4))
        acc = np.zeros((planes, T, P), F32)
        for s in range(batch * heads):
            acc[s % heads if sums_stride_h else 0] += st[s, :P, 1][None, :]
        view[...] = fma32(F32(weight), acc, view.copy() if accumulate else F32(0))
        return 0


def install(setattr_):
    """``_joint_affinity_domain.install`` (CPU tensors pass for device tensors, numpy joint tap and affinity) plus a
    ``FakeJointAttendLib``; ``loads`` counts the calls of ``load_joint_attend``.  Returns ``(engine, joint, affinity, attend, loads)``."""
    import _joint_affinity_domain as JA
    E, joint, aff, _ = JA.install(setattr_)
    lib, loads = FakeJointAttendLib(), []

    def load():
        loads.append(1)
        return lib
    setattr_(E.nat, 'load_joint_attend', load)
    return E, joint, aff, lib, loads
