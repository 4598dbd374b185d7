"""Shared by ``test_attend_domain_cpu.py`` and ``test_gpu_attend_domain.py``: Q / K / V that put the VALUE side of ``daam_attend``
(the second product ``O^T = V^T P^T``, daam_amd/csrc/daam_attend_d64.hip) where a wrong probability slot, a flushed small probability,
a non-zero padding key slot or a lost term moves an output beyond what the two number formats allow, and that bound.

Q and K.  Every element is a multiple of 1/4 with |x| <= 3, so every product is a multiple of 1/16, every partial sum stays below 2^11
and every f32 logit is the same number in any summation order (``tests/_softmax_domain.py``, "Exactness"; pinned by reversing the
head_dim axis in ``tests/test_attend_domain_cpu.py``).  With ``w_m[i] = (-1)^popcount(m & i)`` the Walsh patterns of the low three
index bits (``sd.walsh``: orthogonal to each other and to the all-ones vector over every aligned group of 8 elements):

  K[designed token]  = gk * w_m           tokens 0 / 5 / 41 / 76 with m = 1 / 2 / 3 / 4
  K[every other t]   = kappa              per group of 8 elements: c0 + c5 w_5 + c6 w_6 + c7 w_7, each c in {-1/4, 0, 1/4}
  Q[gapN pixel]      = a_N * w_m + rho    rho per group of 8: r5 w_5 + r6 w_6 + r7 w_7, each r in {-1/4, 0, 1/4}
  Q[tie2 pixel]      = a_t * (w_m + w_m') + rho
  Q[spread pixel]    = N(0,1) rounded to multiples of 1/4, clipped to |x| <= 3

kappa and rho have no component along w_1 .. w_4.  On a gap / tie row the designed token's logit is therefore EXACTLY
``a gk sqrt(d)``, the other designed tokens' logits are exactly 0, and every other token's is ``rho . kappa / sqrt(d)``: N(0, 1/24)
in distribution whatever the head dim (a group contributes ``8 sum_m r_m c_m``), so the minor tokens differ from each other -- two of
them swapped is visible against per-token values -- and stay within about 0.8 nats of 0.

``sd.gain`` moves Q alone and a quarter step of it is 6 nats at head_dim 64 (9.5 at 160): too coarse to tell 16 nats from 20.  ``gains``
therefore picks the designed K rows' ``gk`` per head dim as well: the multiple of 1/4 for which the four levels ``a gk sqrt(d)``
(a a multiple of 1/4 up to 2.25, so that |a + rho| <= 3) come nearest to 8, 12, 16 and 20, inside the windows that make the names true
in fp16 (``GAP_WINDOWS``):

  gap8    minor probabilities about 3e-4                    fp16 normal
  gap12   about 6e-6                                        fp16 subnormal, a hundred ulps
  gap16   about 1e-7                                        one to thirty subnormal ulps (2^-24 = 6e-8), none rounded to zero
  gap20   below 2^-25                                       zero after the rounding itself

Pixel p has kind ``KINDS[p % 13]`` in every step (13 is prime: every lane of a 16-pixel MFMA column group, and every wave, meets every
kind); the first 8 entries hold all six kinds, so a layer of 8 pixels has them too.  The designed token of pixel p at step s is
``DESIGNED[(p // 13 + s) % 4]`` (tie2: that one and the next).

V.  Per token, in the pipeline dtype: ``sign * 2^level[t] * m``, m a random multiple of 1/8 in [1, 2).  ``level`` belongs to the token
and moves on by one token per step, except on ``heavy_minor``, whose levels are tied to the designed tokens:

  plain         level 0
  heavy_minor   level 13 on every token but the four designed ones (level 0): on a gap row the 76 small probabilities carry values
                ten thousand times the dominant token's
  tiny          levels -24 .. -15 on odd tokens (fp16 subnormal values, some rounded to one or two ulps), level 0 on even tokens; the
                designed tokens 5 and 41 are odd
  mixed         levels -20, -8, 0, 6, 12 in turn, the sign alternating with the token: outputs cancel

bf16 takes the same levels (all normal there).

Bound, per element, from the two number formats only:

  |got - want| <= ulp(want) + sum_t ulp(p_t) |v_t| + 77 * 2^-23 * sum_t p_t |v_t|

the output's own rounding; one ulp on every probability (what the project allows a correct softmax: ``tests/_softmax_domain.py``,
``output_slack``); an f32 accumulation of the 77 exact products in another order than the reference's float64."""
import math

import numpy as np

import _softmax_domain as sd
from oracle import heatmap_oracle as ho

TOKENS = sd.TOKENS
HEAD_DIMS = tuple(range(8, 161, 8))
KINDS = ('spread', 'gap8', 'gap12', 'gap16', 'gap20', 'tie2', 'gap12', 'gap16', 'spread', 'gap8', 'gap12', 'gap20', 'tie2')
KIND_NAMES = ('spread', 'gap8', 'gap12', 'gap16', 'gap20', 'tie2')
DESIGNED = (0, 5, 41, 76)
PATTERN = {0: 1, 5: 2, 41: 3, 76: 4}                 # designed token -> Walsh pattern
FREE = (5, 6, 7)                                     # the patterns kappa and rho are made of
GAPS = {'gap8': 8.0, 'gap12': 12.0, 'gap16': 16.0, 'gap20': 20.0}
# The level a gap row may really have.  ln 2^14 = 9.70 (smallest fp16 normal), ln 2^25 = 17.33 (half the smallest subnormal); the minor
# logits stay within 0.9 of 0 (4.5 sigma of N(0, 1/24); tests/test_attend_domain_cpu.py holds the claims themselves)
GAP_WINDOWS = {'gap8': (6.5, 8.8), 'gap12': (10.6, 13.5), 'gap16': (14.2, 16.4), 'gap20': (18.3, 23.0)}
A_MAX = 2.25                                         # |a w + rho| <= 2.25 + 0.75
V_SETS = ('plain', 'heavy_minor', 'tiny', 'mixed')
HEAVY = 13
MIXED_LEVELS = (-20, -8, 0, 6, 12)


def kind_names(hw):
    return np.array([KINDS[p % len(KINDS)] for p in range(hw)])


def designed_token(p, step):
    return DESIGNED[(p // len(KINDS) + step) % len(DESIGNED)]


def gains(d):
    """``(gk, {kind: a})`` of head dim ``d``: see the module docstring."""
    root, best = math.sqrt(d), None
    for gk in np.arange(1, 13) / 4.0:
        a, worst = {}, 0.0
        for kind, level in GAPS.items():
            lo, hi = GAP_WINDOWS[kind]
            fits = [x for x in np.arange(1, int(4 * A_MAX) + 1) / 4.0 if lo <= x * gk * root <= hi]
            if not fits:
                break
            a[kind] = float(min(fits, key=lambda x: abs(x * gk * root - level)))
            worst = max(worst, abs(a[kind] * gk * root - level))
        else:
            if best is None or worst < best[0]:
                best = (worst, float(gk), a)
    assert best is not None, d
    return best[1], best[2]


def _free_part(rng, shape_groups, patterns):
    """[..., groups * 8]: per group of 8 elements ``sum_m c_m w_m`` with c_m in {-1/4, 0, 1/4} for m in ``patterns``."""
    out = np.zeros(shape_groups + (8,), np.float32)
    for m in patterns:
        w = np.ones(8, np.float32) if m == 0 else sd.walsh(m, 8)
        out += (rng.integers(-1, 2, shape_groups)[..., None] / 4.0).astype(np.float32) * w
    return out.reshape(shape_groups[:-1] + (shape_groups[-1] * 8,))


def _typed(x, np_dt):
    assert np.array_equal(sd._round(x, np_dt).astype(np.float32), x)
    return x if ho.is_bf16(np_dt) else x.astype(np_dt)


def build(hw, heads, d, np_dt, n_steps, batch=2, seed=0):
    """``n_steps`` x (q [batch, hw, heads * d], k [batch, 77, heads * d]) in ``np_dt`` (``ho.BF16``: float32 arrays holding bf16
    numbers), and the kind of every pixel."""
    assert d % 8 == 0 and 8 <= d <= 160
    names = kind_names(hw)
    gk, a = gains(d)
    a_tie = min(a['gap12'], 1.0)                      # |a (w + w') + rho| <= 2 + 0.75
    rng = np.random.default_rng([seed, hw, heads, d, batch])
    steps = []
    for s in range(n_steps):
        q = np.clip(np.round(4.0 * rng.standard_normal((batch, hw, heads, d))) / 4.0, -3.0, 3.0).astype(np.float32)
        rho = _free_part(rng, (batch, hw, heads, d // 8), FREE)
        for p in np.nonzero(names != 'spread')[0]:
            i = (p // len(KINDS) + s) % len(DESIGNED)
            w = sd.walsh(PATTERN[DESIGNED[i]], d)
            if names[p] == 'tie2':
                row = a_tie * (w + sd.walsh(PATTERN[DESIGNED[(i + 1) % len(DESIGNED)]], d))
            else:
                row = a[names[p]] * w
            q[:, p] = row + rho[:, p]
        k = _free_part(rng, (batch, TOKENS, heads, d // 8), (0,) + FREE)
        for t, m in PATTERN.items():
            k[:, t] = gk * sd.walsh(m, d)
        assert np.abs(q).max() <= 3.0 and np.abs(k).max() <= 3.0
        steps.append((_typed(q.reshape(batch, hw, heads * d), np_dt), _typed(k.reshape(batch, TOKENS, heads * d), np_dt)))
    return steps, names


def levels(v_set, step):
    """(level, sign or None) per token at ``step``; a sign of None is drawn at random per element."""
    t = (np.arange(TOKENS) + step) % TOKENS
    if v_set == 'plain':
        return np.zeros(TOKENS, int), None
    if v_set == 'heavy_minor':
        return np.where(np.isin(np.arange(TOKENS), DESIGNED), 0, HEAVY), None
    if v_set == 'tiny':
        return np.where(t % 2 == 1, -24 + (t // 2) % 10, 0), None
    assert v_set == 'mixed', v_set
    return np.array(MIXED_LEVELS)[t % len(MIXED_LEVELS)], np.where(t % 2 == 0, 1.0, -1.0)


def values(v_set, heads, d, np_dt, n_steps, batch=2, seed=0):
    """V [batch, 77, heads * d] of every step, in ``np_dt``."""
    rng = np.random.default_rng([seed, V_SETS.index(v_set), heads, d, batch, 4 if ho.is_bf16(np_dt) else 3])
    out = []
    for s in range(n_steps):
        level, sign = levels(v_set, s)
        shape = (batch, TOKENS, heads * d)
        m = 1.0 + rng.integers(0, 8, shape) / 8.0
        sg = np.where(rng.integers(0, 2, shape) == 0, 1.0, -1.0) if sign is None else sign[None, :, None]
        v = sd._round((sg * m * 2.0 ** level[None, :, None]).astype(np.float32), np_dt)       # fp16 subnormals round here
        out.append(v if ho.is_bf16(np_dt) else v.astype(np_dt))
    return out


def accumulation_slack(probs, v_bh):
    """f32 accumulation of the 77 exact products in any order: ``77 * 2^-23 * sum_t p_t |v_t|``, [BH, hw, d]."""
    return TOKENS * 2.0 ** -23 * np.matmul(np.asarray(probs, np.float64), np.abs(np.asarray(v_bh, np.float64)))


def bound(want, probs, v_bh, np_dt):
    return sd.ulp_of(want, np_dt) + sd.output_slack(probs, v_bh, np_dt) + accumulation_slack(probs, v_bh)


def reference(q, k, v, heads, scale, np_dt):
    """Oracle of one call: ``dict(probs [BH, hw, 77], want [BH, hw, d], bound, vh)`` in float64."""
    qh, kh, vh = (sd.to_bh(np.asarray(x, np.float32), heads) for x in (q, k, v))
    probs = np.asarray(ho.attention_probs(qh, kh, scale, np_dt), np.float64)
    want = np.asarray(ho.attention_output(qh, kh, vh, scale, np_dt), np.float64)
    assert np.isfinite(want).all() and np.isfinite(probs).all()
    return dict(probs=probs, want=want, bound=bound(want, probs, vh, np_dt), vh=vh.astype(np.float64), qh=qh, kh=kh)


def worst_by_kind(got_bh, ref, names):
    """``{kind: (worst err / bound, (head, pixel, element))}`` of an output [BH, hw, d] against ``reference``'s dict."""
    ratio = np.abs(np.asarray(got_bh, np.float64) - ref['want']) / ref['bound']
    out = {}
    for kind in KIND_NAMES:
        sel = names == kind
        if sel.any():
            part = np.where(sel[None, :, None], ratio, -1.0)
            at = np.unravel_index(int(part.argmax()), part.shape)
            out[kind] = (float(part[at]), tuple(int(i) for i in at))
    return out


def report(worst):
    return ', '.join(f'{kind} {r:.3f}' for kind, (r, _) in worst.items())


def rect_sums(probs_steps, acc_np, h, w):
    """Running sums [kept heads, 77, h, w] of the given per-step probabilities [BH, h * w, 77]: the kept half (trace.py:240), one
    add per step in the sum dtype (heatmap.py:156)."""
    raw = ho.RawMaps(acc_np)
    for probs in probs_steps:
        kept = sd.kept(np.asarray(probs, np.float32))
        for head in range(kept.shape[0]):
            raw.update(1, 0, head, np.ascontiguousarray(kept[head].T).reshape(TOKENS, h, w))
    return np.stack([m for _, m in raw]).astype(np.float64)
