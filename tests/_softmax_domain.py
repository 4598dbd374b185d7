"""Shared by ``test_softmax_domain_cpu.py`` and ``test_gpu_softmax_domain.py``: Q / K whose pixels ("rows") put the softmax of the
tap kernels and of ``daam_attend`` on every side of its shortcut, and the classifier that says on which side a row is.

The shortcut (daam_amd/csrc/daam_tap16_softmax.h, daam_tap_common.h): the exponentials are taken of the logits themselves -- of the
logits minus token 0's in ``tap_mfma_kernel`` -- and a pixel is redone with its row maximum only when its sum leaves
[2^-100, 2^100].  A row is therefore

  plain   -100 <= log2 sum_t exp(x_t) <= 100      the shortcut's result is kept
  over    above 100 (past 127 the f32 sum is inf)   redone
  under   below -100 (past -126 the sum is 0)       redone

with ``x_t - x_0`` in place of ``x_t`` for the token-0 flavour (``shifted=True``), whose sum is at least 1: it has no ``under``.

Construction.  With ``1`` the all-ones vector of the head_dim axis and ``w_m[i] = (-1)^popcount(m & i)`` (Walsh patterns of the low
three index bits: orthogonal to ``1`` and to each other whenever head_dim is a multiple of 8),

  K[token t]   = BETA * 1 + GAMMA * w_m          for the designed tokens: 5 (m = 1), 0 (m = 2), 76 (m = 3), 20 and 41 (m = 4),
                                                  9, 30 and 63 (m = 5)
               = BETA * 1 + kappa                every other token; kappa = N(0,1) rounded to multiples of 1/4, |kappa| <= 3
  Q[extreme p] = a * w_m + b * 1                 a, b multiples of 1/4
  Q[plain p]   = N(0,1) minus the row's mean     (so that the uniform part of K moves a plain row by next to nothing)

K is "uniformly negative plus a random part" in every step (BETA = -3): a row with b > 0 has EVERY logit near ``-3 b sqrt(d)``, in
every head, a row with b < 0 every logit that far above zero, and a row with b = 0 does not see BETA at all: its logit of the
designed token of pattern m is ``3 a sqrt(d)`` and every other logit is ``a * N(0,1)``.  ``gain(level)`` turns a wanted logit level
into the multiple of 1/4 nearest ``level / (3 sqrt(d))`` (exactly 2 / 4 / 8 for 48 / 96 / 192 at head_dim 64).

Exactness.  On an extreme row every product q_i k_i is a multiple of 1/16 and every partial sum stays below 2^14: all of them are
exact in f32, in any summation order (numpy's, the MFMA's k-steps, the f32 FMAs of the any-shape kernel).  The f32 logit before the
rounding to the pipeline dtype is then the same number everywhere (one more f32 multiply by the scale when that is no power of
two), and so is the rounded one: the expected sums of an extreme row do not hang on a rounding flip of a logit whose ulp is 2^-5
(fp16 near 48) or 2^-1 (bf16 near 96).  ``tests/test_softmax_domain_cpu.py`` pins this by reversing the head_dim axis.

Rows: class ``SLOTS[p % 17]`` for pixel p in every step (17 is prime: every lane of a 16-pixel MFMA column group, and every wave,
meets every class); the levels of the ``over`` and ``under`` slots rotate with the step."""
import math

import numpy as np

from oracle import heatmap_oracle as ho

TOKENS = 77
BATCH = 2
HWS = (256, 576)                    # exact tiles / a partial tile and waves outside the tensor
BETA = -3.0
GAMMA = 3.0
DESIGNED = {5: 1, 0: 2, 76: 3, 20: 4, 41: 4, 9: 5, 30: 5, 63: 5}      # token -> Walsh pattern
OVER_LEVELS = (80, 96, 192, 48)     # sum 2^115 (finite), inf, inf, 2^69 (below the switch: such a row classifies as plain)
UNDER_LEVELS = (112, 88, 192)       # sum 0 or subnormal, 2^-120 (every exponential still normal), 0
T0_LEVEL = 112                      # token 0 this far above / below every other token
SLOTS = ('plain', 'over', 'under', 't0_low', 'plain', 'over', 'under', 't0_high', 'plain', 'over', 'under', 'tie2', 'last', 'over',
         'tie3', 'over_all', 'plain')
PLAIN, OVER, UNDER = 0, 1, 2
CLASS_NAMES = ('plain', 'over', 'under')
SWITCH = 100.0                      # |log2 sum| beyond which the kernels redo a row


def walsh(m, d):
    i = np.arange(d)
    return np.where(np.array([bin(m & v).count('1') for v in i]) % 2 == 0, 1.0, -1.0).astype(np.float32)


def gain(level, d):
    return round(4.0 * level / (GAMMA * math.sqrt(d))) / 4.0


def slot_names(hw):
    return np.array([SLOTS[p % len(SLOTS)] for p in range(hw)])


def _extreme_row(name, nth, step, d):
    """(pattern, a, b) of the ``nth`` slot of its name at ``step``."""
    if name == 'over':
        return 1, gain(OVER_LEVELS[(nth + step) % len(OVER_LEVELS)], d), 0.0
    if name == 'under':
        return 1, 0.0, gain(UNDER_LEVELS[(nth + step) % len(UNDER_LEVELS)], d)
    return {'t0_low': (2, -gain(T0_LEVEL, d), 0.0), 't0_high': (2, gain(T0_LEVEL, d), 0.0), 'tie2': (4, gain(96, d), 0.0),
            'tie3': (5, gain(80, d), 0.0), 'last': (3, gain(96, d), 0.0), 'over_all': (1, 0.0, -gain(96, d))}[name]


def _round(x, np_dt):
    return ho.round_bf16(x) if ho.is_bf16(np_dt) else x.astype(np_dt)


def build(hw, heads, d, np_dt, n_steps, seed=0):
    """``n_steps`` x (q [BATCH, hw, heads * d], k [BATCH, 77, heads * d]) in ``np_dt`` (``ho.BF16``: float32 arrays holding bf16
    numbers), and the slot name of every pixel."""
    assert d % 8 == 0
    names = slot_names(hw)
    nth = {n: np.cumsum(np.array(SLOTS) == n) - 1 for n in set(SLOTS)}          # which of its name's slots a slot is
    rng = np.random.default_rng([seed, hw, heads, d])
    steps = []
    for s in range(n_steps):
        q = rng.standard_normal((BATCH, hw, heads, d)).astype(np.float32)
        q -= q.mean(-1, keepdims=True)
        q = _round(q, np_dt).astype(np.float32)
        for p in np.nonzero(names != 'plain')[0]:
            slot = p % len(SLOTS)
            m, a, b = _extreme_row(SLOTS[slot], nth[SLOTS[slot]][slot], s, d)
            q[:, p] = a * walsh(m, d) + b
        kappa = np.clip(np.round(4.0 * rng.standard_normal((BATCH, TOKENS, heads, d))) / 4.0, -3.0, 3.0).astype(np.float32)
        k = BETA + kappa
        for t, m in DESIGNED.items():
            k[:, t] = BETA + GAMMA * walsh(m, d)
        q, k = q.reshape(BATCH, hw, heads * d), k.reshape(BATCH, TOKENS, heads * d)
        assert np.array_equal(_round(q, np_dt), q) and np.array_equal(_round(k, np_dt), k)
        steps.append((q if ho.is_bf16(np_dt) else q.astype(np_dt), k if ho.is_bf16(np_dt) else k.astype(np_dt)))
    return steps, names


def to_bh(x, heads):
    b, s, c = x.shape
    d = c // heads
    return np.ascontiguousarray(x.reshape(b, s, heads, d).transpose(0, 2, 1, 3)).reshape(b * heads, s, d)


def rounded_logits(q_bh, k_bh, scale, np_dt, upcast=False):
    """The logits as ``ho.attention_probs`` forms them: f32 accumulation, the scale in f32, one rounding to the pipeline dtype
    (none with ``upcast``).  [BH, hw, 77] float32."""
    acc = np.matmul(q_bh.astype(np.float32), np.swapaxes(k_bh.astype(np.float32), -1, -2)) * np.float32(scale)
    return acc if upcast else _round(acc, np_dt).astype(np.float32)


def log2_sum(logits, shifted=False):
    """float64 ``log2 sum_t exp(x_t)`` (``exp(x_t - x_0)`` with ``shifted``) per row."""
    x = logits.astype(np.float64)
    if shifted:
        x = x - x[..., :1]
    m = x.max(-1)
    return (m + np.log(np.exp(x - m[..., None]).sum(-1))) / math.log(2.0)


def classify(logits, shifted=False):
    v = log2_sum(logits, shifted)
    return np.where(v > SWITCH, OVER, np.where(v < -SWITCH, UNDER, PLAIN))


def kept(x_bh):
    """The half of batch * heads the tap keeps (trace.py:240)."""
    return x_bh[x_bh.shape[0] // 2:]


def row_classes(steps, heads, scale, np_dt, shifted=False, upcast=False):
    """[steps, kept heads, hw]: PLAIN / OVER / UNDER of every row the tap keeps."""
    return np.stack([classify(kept(rounded_logits(to_bh(q, heads), to_bh(k, heads), scale, np_dt, upcast)), shifted) for q, k in steps])


def pixel_classes(per_step):
    """[kept heads, hw]: the class of a pixel's running sum -- OVER if any of its steps is, else UNDER if any is, else PLAIN."""
    return np.where((per_step == OVER).any(0), OVER, np.where((per_step == UNDER).any(0), UNDER, PLAIN))


def softmax64(logits, np_dt):
    """float64 softmax of the given logits, rounded once to the pipeline dtype."""
    x = logits.astype(np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return _round((e / e.sum(-1, keepdims=True)).astype(np.float32), np_dt)


def worst_by_class(got, want, classes):
    """``{class name: (max-abs error, (head, pixel) of the worst row, rows)}`` for sums ``[..., kept heads, 77, side, side]`` (any
    leading axes are windows) and ``classes`` [kept heads, hw]."""
    heads, hw = classes.shape
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).reshape(-1, heads, TOKENS, hw).max((0, 2))
    out = {}
    for c, name in enumerate(CLASS_NAMES):
        sel = classes == c
        if sel.any():
            flat = np.where(sel, err, -1.0)
            h, p = np.unravel_index(int(flat.argmax()), flat.shape)
            out[name] = (float(flat[h, p]), (int(h), int(p)), int(sel.sum()))
    return out


# ---- daam_attend outputs -----------------------------------------------------------------------------------------------------
def attend_values(hw, heads, d, np_dt, n_steps):
    """V [BATCH, 77, heads * d] of every step: N(0,1) in the pipeline dtype."""
    rng = np.random.default_rng([hw, d, 4 if ho.is_bf16(np_dt) else 3])
    return [_round(rng.standard_normal((BATCH, TOKENS, heads * d)).astype(np.float32), np_dt) for _ in range(n_steps)]


def ulp_of(x, np_dt):
    """Spacing of the pipeline dtype at |x| (float64 array)."""
    x = np.abs(np.asarray(x, np.float64))
    if ho.is_bf16(np_dt):
        return 2.0 ** (np.floor(np.log2(np.maximum(x, 2.0 ** -126))) - 7)
    return np.spacing(x.astype(np.float16)).astype(np.float64)


def output_slack(probs, v_bh, np_dt):
    """What one ulp on every probability of a row can move that row's outputs by: ``sum_t ulp(p_t) |v_t|``, [BH, hw, d]."""
    return np.matmul(ulp_of(probs, np_dt), np.abs(np.asarray(v_bh, np.float64)))


def emulate_fast_probs(logits, np_dt):
    """The kernels' fast softmax after its redo, in numpy: ``e = 2^(f32(x L - m L))`` (one f32 rounding of the exponent, as the
    FMA leaves it), f32 sum, ``p = dtype(e * (1 / sum))``.  Differs from the oracle's f32 softmax the way any other correct f32
    implementation does: by a probability rounded the other way now and then."""
    L = float(np.float32(1.44269502162933349609375))
    x = np.asarray(logits, np.float64)
    nml = np.float32(-x.max(-1, keepdims=True) * L).astype(np.float64)
    e = np.exp2((x * L + nml).astype(np.float32).astype(np.float64)).astype(np.float32)
    tot = e.sum(-1, keepdims=True, dtype=np.float32)
    return _round(e * (np.float32(1) / tot), np_dt)


def emulate_output(probs, v_bh, np_dt):
    """``dtype(f32(sum_t p_t v_t))``: the value product accumulated wide and rounded once."""
    return _round(np.matmul(np.asarray(probs, np.float64), np.asarray(v_bh, np.float64)).astype(np.float32), np_dt)
