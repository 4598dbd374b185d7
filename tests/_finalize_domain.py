"""Shared by ``test_finalize_domain_cpu.py`` and ``test_gpu_finalize_domain.py``: "levelled planes" whose token rows differ by
up to 2^21 in magnitude, the float64 reference of the finalize (bicubic -> clamp -> mean over keys), the per-token-row error
metric and the two contracts a finalize kernel is held to.

Levelled planes.  ``[2 * heads, side * side, 77]`` per layer, unconditional half zero.  The kept half is ``exp(standard_normal)``
(log-normal: heavy-tailed, a few elements 100 times the median), token ``t`` multiplied by ``2^-(3 * (t % 8))`` -- neighbouring token
rows sit 8 x apart, rows 0 and 7 a factor 2^21 -- and the whole set by ``2^k``.  The signed variant flips random signs (the clamp
matters).  Everything after the draw is a multiplication by a power of two, so rounding to the sums' dtype commutes with the scale
unless a value leaves the dtype's normal range; ``homogeneous`` tells.

Contracts, per token row ``t`` with ``err_t = max_pixels |got[t] - want64[t]|`` and ``rowmax_t = max_pixels |want64[t]|``:

  * exact-f32 routes (same-size, x4, LDS x2, x0.5, any-size kernel and their grouped forms):  ``err_t <= 2^-19 * rowmax_t``.
    The f32 four-tap sums of both passes, at most 6 f32 adds over the keys and (on the MFMA routes) the 2^-22 hi + lo split come to
    under 2^-20 of the row's maximum; one factor of two is margin.
  * MFMA x2 routes (``finalize_up32_pipe_kernel``, ``finalize_up32_mfma_kernel``, ``finalize_up32_same_kernel``):
    ``err_t <= 2^-19 * rowmax_t + 2^-23``, planes inside ``|v| <= 2^15``.  These kernels feed f32 numbers to the fp16 matrix pipe as
    ``hi = fp16(v)``, ``lo = fp16(v - hi)``; ``lo`` is an fp16 subnormal whenever ``|v| < 2^-3``, so the split's error is an ABSOLUTE
    half subnormal ulp, 2^-25.  The x2 tap weights' absolute sum is 1.28 per pass and there are at most two splits (the plane for
    f32 sums, the intermediate T for every dtype): 2.92 * 2^-25 < 2^-23 per map element, which the mean over keys does not grow.
    The floor does not scale with the planes.
"""
import math

import numpy as np

from oracle import heatmap_oracle as ho

TOKENS = 77
N_LEVELS = 8
LEVEL_STEP = 3                       # token t sits at 2^-(3 * (t % 8))
REL = 2.0 ** -19                     # relative part of both contracts (of the token row's maximum)
FLOOR = 2.0 ** -23                   # absolute floor of the MFMA x2 routes, not scaled by k
ORACLE_F32_REL = 2.0 ** -21          # the f32 numpy oracle against the float64 one, per token row
DOMAIN_MAX = 2.0 ** 15               # documented bound of the MFMA x2 routes; fp16 sums cannot hold much more (65504) on any route

SIDES = [(64,), (32,), (16,), (128, 64), (16, 32, 64), (8,), (24, 48)]
DTYPES = ['float16', 'bfloat16', 'float32']
VARIANTS = ['nonneg', 'signed']
K_EXACT = [-20, -10, 0, 6, 12]       # + 40 for bf16 / f32 sums
K_MFMA = [-10, 0, 6, 12]
HEADS = 2                            # kept heads per layer: at most 3 layers x 2 = 6 keys in one mean


def out_side_of(sides):
    return 96 if 24 in sides else 64


def factor_of(side, out_side):
    return out_side // side if side <= out_side else 0


def token_levels():
    return 2.0 ** -(LEVEL_STEP * (np.arange(TOKENS) % N_LEVELS)).astype(np.float64)


def draw_planes(sides, variant, heads=HEADS, seed=0):
    """The k = 0 planes of every layer as float32 (not yet rounded to the sums' dtype): ``[2 * heads, side * side, 77]`` each."""
    rng = np.random.default_rng([seed, len(sides), sides[0], VARIANTS.index(variant)])
    lev = token_levels().astype(np.float32)
    out = []
    for side in sides:
        x = np.exp(rng.standard_normal((heads, side * side, TOKENS))).astype(np.float32)
        if variant == 'signed':
            x *= rng.choice(np.float32([-1.0, 1.0]), size=x.shape)
        out.append(np.concatenate([np.zeros_like(x), x * lev]))
    return out


def round_to(planes, dtype):
    """To the sums' dtype as the oracle carries it: float16 / float32 arrays, bf16 as float32 holding bf16 numbers."""
    if dtype == 'bfloat16':
        return ho.round_bf16(planes)
    with np.errstate(over='raise'):
        return np.asarray(planes, np.float32).astype(dtype)


def scale_exp(base, k, limit=None):
    """The exponent really applied for a requested ``k``: lowered until ``max|v| * 2^k <= limit`` (the MFMA routes' domain, the fp16
    range), so that the draw is divided by a power of two and nothing else about it changes."""
    if limit is None:
        return k
    top = max(float(np.abs(b).max()) for b in base)
    return min(k, int(math.floor(math.log2(limit / top))))


def scaled_planes(base, k, dtype):
    """``round(base * 2^k)`` per layer, and whether that equals ``round(base) * 2^k`` everywhere (no value became subnormal,
    underflowed or overflowed in the sums' dtype), i.e. whether the k = 0 reference times 2^k is this input's reference."""
    s = np.float32(2.0 ** k)
    got = [round_to(b * s, dtype) for b in base]
    homogeneous = all(np.array_equal(g.astype(np.float64), round_to(b, dtype).astype(np.float64) * 2.0 ** k)
                      for g, b in zip(got, base))
    return got, homogeneous


def raw_keys(planes, sides, out_side):
    """``[((factor, layer, head), [77, side, side])]`` as ``ho.global_heat_map`` takes them, from per-layer ``[2 * heads, hw, 77]``."""
    raw = []
    for layer, (side, p) in enumerate(zip(sides, planes)):
        kept = ho.unravel(p)
        raw += [((factor_of(side, out_side), layer, h), kept[h]) for h in range(kept.shape[0])]
    return raw


def reference64(planes, sides, out_side, **kw):
    return ho.global_heat_map(raw_keys(planes, sides, out_side), out_side * out_side, dtype=np.float64, **kw)


def row_errors(got, want64):
    """``(err_t, rowmax_t)`` over the pixels of every token row."""
    got = np.asarray(got, np.float64).reshape(len(want64), -1)
    want = np.asarray(want64, np.float64).reshape(len(want64), -1)
    return np.abs(got - want).max(1), np.abs(want).max(1)


def contract_bound(rowmax, mfma):
    return REL * rowmax + (FLOOR if mfma else 0.0)


def worst(err, rowmax, mfma=False):
    """What to write down about a result.  Exact routes: the largest ``err_t / rowmax_t`` (rows whose reference is all zero left out)
    and the largest ``err_t``.  MFMA routes: the largest ``err_t / rowmax_t`` over the rows whose relative allowance is at least the
    floor (``2^-19 * rowmax_t >= 2^-23``: the relative regime) and the largest ``err_t`` over the other rows (the floor regime: the
    observed absolute floor)."""
    rel_rows = rowmax > 0
    abs_rows = np.ones_like(rel_rows)
    if mfma:
        rel_rows = REL * rowmax >= FLOOR
        abs_rows = ~rel_rows
    return (float((err[rel_rows] / rowmax[rel_rows]).max()) if rel_rows.any() else 0.0,
            float(err[abs_rows].max()) if abs_rows.any() else 0.0)


def assert_contract(got, want64, mfma, what):
    """Both contracts exactly as stated above; returns ``worst(err, rowmax, mfma)``."""
    assert np.isfinite(np.asarray(got)).all(), f'{what}: non-finite output'
    err, rowmax = row_errors(got, want64)
    bound = contract_bound(rowmax, mfma)
    bad = np.nonzero(err > bound)[0]
    rel, ab = worst(err, rowmax, mfma)
    assert bad.size == 0, (f'{what}: {bad.size} token rows outside the {"MFMA" if mfma else "exact"} contract; worst rows ' +
                           ', '.join(f't={t} err {err[t]:.3e} = 2^{math.log2(err[t]):.1f} (rowmax {rowmax[t]:.3e}, bound {bound[t]:.3e})'
                                     for t in bad[np.argsort(-(err[bad] / np.maximum(bound[bad], 1e-300)))][:4]))
    return rel, ab


# ---- the hi + lo split of the MFMA x2 kernels, emulated (everything else exact in float64) -----------------------------------
def split_fp16(x):
    """``fp16(x) + fp16(x - fp16(x))`` as a float64 array: what reaches the fp16 matrix pipe for an f32 number x."""
    x = np.asarray(x, np.float64)
    hi = x.astype(np.float16).astype(np.float64)
    return hi + (x - hi).astype(np.float16).astype(np.float64)


def emulate_mfma_x2(planes32, dtype):
    """The global map of 32 x 32 keys ``planes32`` ([2 * heads, 1024, 77], already rounded to ``dtype``) -> 64 x 64 as an MFMA x2 kernel
    forms it, with the two splits as the only error: the plane itself for f32 sums (fp16 / bf16 planes enter the matrix pipe as they
    are), and T between the passes for every dtype."""
    kept = ho.unravel(np.asarray(planes32)).astype(np.float64)               # [heads, 77, 32, 32]
    idx, w = ho.bicubic_taps(32, 64, np.float64)
    total = 0.0
    for p in kept:
        if dtype == 'float32':
            p = split_fp16(p)
        t = sum(p[..., :, idx[:, b]] * w[:, b] for b in range(4))             # [77, 32, 64]
        t = split_fp16(t)
        up = sum(t[..., idx[:, a], :] * w[:, a][:, None] for a in range(4))   # [77, 64, 64]
        total = total + np.maximum(up, 0)
    return total / len(kept)
