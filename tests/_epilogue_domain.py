"""Shared by ``test_epilogue_domain_cpu.py`` and ``test_gpu_epilogue_domain.py``: planes that put the word-map epilogue
(``normalize_kernel``, ``word_mean_kernel``, ``word_expand[_rect]_kernel``, ``word_post_kernel``, ``mask_overlap_kernel`` in
daam_amd/csrc/daam_kernels.hip / daam_word_expand_body.inc, and their batched restatement daam_word_masks.hip) where a wrong tap, a
wrong weight, a lane missed by the min / max or a dropped epsilon moves a value beyond what f32 arithmetic allows; a float64 oracle of
every step; the per-element bounds; and an f32 numpy emulation of every kernel, in its operation order, whose switches are the
mutants the CPU file proves the cases catch.

Oracle.  Source coordinates and cubic coefficients are computed in f32 in the operation order of ``cubic_coeffs`` and the expand
body (``sc = f32(in) / f32(out)``, ``src = sc * (dst + 0.5f) - 0.5f``, ``t = src - floor(src)``, the Horner forms, ``u = 1 - t`` and
``x3 = u + 1``, no contraction): the reference computes them the same way, so they are INPUTS of the comparison, not part of its
error (``coefficients64`` gives them in float64 for the CPU file, which holds the f32 ones to them).  Everything after them is
float64: the 16 products and their sums, the word mean, both normalisations with their epsilons as the f32 constants
``f32(1e-6)`` / ``f32(1e-8)``, the comparison with ``f32(threshold)``.

Bounds, with ``u = 2^-24`` (one f32 rounding is a relative error of at most u; ``ulp(x)`` is the spacing of f32 at x, >= 2 u |x| / 2):

  resize      ``ulp(want) + 8 u S``, ``S = sum_y sum_x |wy| |wx| |v|``.  A row is four products and three additions, the column
              pass the same on the four rows: seven roundings each, but a single term passes only the four on its own path (its
              product and at most three additions) in each pass, so every |wy wx v| carries at most ``(1 + u)^8 - 1`` -- K = 8
              (taken as ``8 u / (1 - 8 u)``).  ``ulp(want)`` is the issue's allowance on the result itself.  Identity sizes are a
              copy: the bound is 0.
  word mean   ``(n + 1) u sum|v| / n``: n - 1 additions (the first adds to 0) and one division, each term passes at most n.
  normalise   c the content rows 1 .. n_rows - 2, s their sum plus 1e-6: n_rows - 2 roundings in s, each at most u times a partial
              sum <= S = sum|c| + 1e-6, so ``|s' - s| <= e = (n_rows - 2) u S`` and ``|v / s' - v / s| <= |want| e / (|s| - e)``;
              the division is given the rest of n_rows + 2 (4 u of its result), which on a non-negative plane (S = s) makes this the issue's
              ``(n_rows + 2) u |want|`` (the CPU file asserts that it is); on a signed plane s may cancel, the bound
              grows with S / |s|, and where e reaches |s| / 2 the pixel is ``free`` (nothing is asserted there; the CPU file caps
              how many there are).
  min-max     with ``b`` the resize bound: the kernel's lo is the exact minimum of ITS values, so ``lo' in [min(want - b),
              min(want + b)]``: ``b_lo`` is the larger distance from ``lo``; ``b_hi`` likewise.  With q = (v - lo) / d,
              d = hi - lo + 1e-8:  ``|q' - q| <= (b + b_lo + |q| (b_hi + b_lo)) / (d - b_hi - b_lo) + 3 ulp(q)`` -- the three ulps
              hold the subtraction, the two roundings of d and the division (four roundings of at most u = half an ulp).
              Where this exceeds 2^-10 anywhere (or d - b_hi - b_lo <= 0) the PLANE is ill-conditioned, for the reference too
              (a constant plane, a 1 x 1 source, a single output pixel: a range of a few ulps beside 1e-8): then only the
              range rule holds.  The range rule holds always and is asserted always: v' >= lo' and v' - lo' <= hi' - lo' <=
              fl(hi' - lo' + 1e-8) in f32, so every output is finite and in [0, 1] (inside the issue's [-bound, 1 + bound]).
  threshold   a pixel is ambiguous when ``|want - f32(threshold)| <= bound`` (the bound of the value compared: resize under
              ``absolute``, min-max otherwise); every other pixel must match ``want > f32(threshold)`` exactly.  Where the bound
              is 0 (an ``absolute`` copy at identity sizes) nothing is ambiguous: a value equal to the threshold must give 0,
              which is how ``>=`` for ``>`` is caught (``dyadic_plane``).
  overlap     after a resize: D = pixels with ``want - 1 > bound``, Amb = pixels with ``|want - 1| <= bound``; each of sum(a b)
              and sum(a) lies in ``[sum_D, sum_D + sum_Amb]`` (b is binary, the sums are integers below 2^24: exact in any
              order), sum(b) is exact.  Same size, soft: ``sum|terms| (waves + 6) u`` (one product, six shuffle additions, one
              atomic addition per wave).

Caps (asserted by the CPU file on the oracle alone, over every case of the GPU file): ambiguous pixels are at most 2e-3 of a case's
pixels; ill-conditioned min-max cases are only the ``constant`` kind, a 1 x 1 source (a constant plane whatever its kind) and a
single output pixel (its range is 0; the kernel's answer there is exactly 0, which the GPU file asserts)."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
K_RESIZE = 8.0 * U / (1.0 - 8.0 * U)
EPS_NORM, EPS_RANGE = F32(1e-6), F32(1e-8)
ILL = 2.0 ** -10
AMBIGUOUS_CAP = 2e-3
A32 = F32(-0.75)

# source -> output of expand_word_map (the issue's table)
SIZE_SETS = [((64, 64), (128, 128)), ((64, 64), (200, 333)), ((16, 24), (37, 53)), ((48, 48), (32, 32)), ((12, 20), (12, 20)),
             ((1, 1), (5, 7)), ((2, 2), (9, 9)), ((8, 8), (3, 3)), ((8, 8), (1, 1)), ((24, 16), (16, 24)), ((128, 128), (256, 256))]
EXPAND_KINDS = ('real', 'signed', 'negative', 'levels', 'tiny', 'peak_last', 'peak_first', 'constant')
# (absolute, threshold) of every expand case, and the extra thresholds of a few
MODES = ((False, None), (True, None), (False, 0.4), (True, 0.4))
EXTRA_THRESHOLDS = (-0.25, 1.0, 1.5)
EXTRA_CASES = [(((16, 24), (37, 53)), 'signed'), (((64, 64), (128, 128)), 'negative'), (((64, 64), (200, 333)), 'levels')]
NORMALIZE_ROWS = (1, 2, 3, 9, 77)
NORMALIZE_KINDS = ('plain', 'real', 'signed', 'tiny', 'zero_content')
NORMALIZE_PLANES = ((1, 1), (7, 9), (16, 16), (1, 257), (64, 64), (32, 128))          # h w = 1, 63, 256, 257, 4096, 4096
WORD_KINDS = ('real', 'signed', 'levels')
WORD_LISTS = {'one': [4], 'three': [2, 3, 5], 'all content': list(range(1, 76)), 'repeats': [3, 3, 7, 3, 9, 7],
              'descending': [60, 41, 40, 7, 2], '77 indices': list(range(77)), '80 with repeats': list(range(77)) + [5, 5, 76]}
MASK_SIZES = [((16, 24), (37, 53)), ((64, 64), (200, 333)), ((24, 16), (16, 24))]
MASK_KINDS = ('negative', 'peak_last', 'peak_first', 'signed', 'tiny')
OVERLAP_SHAPES = [((17, 23), (40, 31)), ((64, 64), (200, 333)), ((96, 96), (64, 64)), ((64, 64), (512, 512)), ((1, 1), (9, 9))]
OVERLAP_KINDS = ('soft', 'blocks', 'levels')


def ulp(x):
    """Spacing of f32 at |x| (float64 in, float64 out); the smallest subnormal at 0."""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return np.maximum(2.0 ** (e - 23), 2.0 ** -149)


# ---- planes ----------------------------------------------------------------------------------------------------------------------------
def planes(kind, rows, h, w, seed=0):
    """f32 [rows, h, w] of ``kind`` (the issue's table)."""
    rng = np.random.default_rng([seed, rows, h, w, sum(map(ord, kind))])
    n = rng.standard_normal((rows, h, w))
    if kind == 'plain':
        out = np.abs(n)
    elif kind == 'real':
        yy, xx = np.mgrid[0:h, 0:w]
        out = np.empty((rows, h, w))
        for r in range(rows):
            cy, cx, s = rng.uniform(0, max(h - 1, 1)), rng.uniform(0, max(w - 1, 1)), 0.15 * max(h, w) + 1.0
            bump = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            out[r] = 10.0 ** rng.uniform(-4, -2) * (0.2 + bump + 0.05 * np.abs(n[r]))
        out[0] = 50.0 + np.abs(n[0])
        if rows > 1:
            out[-1] = 1.0 + 0.1 * np.abs(n[-1])
    elif kind == 'signed':
        out = np.where(rng.random((rows, h, w)) < 1 / 16, -0.0, n)
    elif kind == 'negative':
        out = -(np.abs(n) + 0.01)
    elif kind == 'levels':
        e = rng.integers(-20, 4, (rows, (h + 1) // 2, (w + 1) // 2))
        out = np.abs(n) * 2.0 ** np.repeat(np.repeat(e, 2, 1), 2, 2)[:, :h, :w]
    elif kind == 'tiny':
        out = np.abs(n) * 2.0 ** -30
    elif kind == 'zero_content':
        out = np.abs(n)
        out[1:-1] = np.where(rng.random((h, w)) < 1 / 8, 0.0, out[1:-1])
    elif kind in ('peak_last', 'peak_first', 'constant'):
        out = np.full((rows, h, w), 0.25)
        if kind == 'peak_last':
            out[:, -1, -1] = 8.0
        elif kind == 'peak_first':
            out[:, 0, 0] = -8.0
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(out, dtype=F32)


def dyadic_plane(h, w, seed=0):
    """Multiples of 1/8 in [0, 1]: an eighth of the pixels equal the threshold 0.5 exactly."""
    return (np.random.default_rng([seed, h, w, 8]).integers(0, 9, (h, w)) / 8.0).astype(F32)


def word_plane(kind, h, w, seed=0):
    """The [h, w] plane the expand cases resize: a content row of ``planes``."""
    return planes(kind, 4, h, w, seed)[2]


# ---- coefficients ---------------------------------------------------------------------------------------------------------------------
def cubic_weights(t, dtype=F32, a=-0.75):
    """``cubic_coeffs`` (daam_kernels.hip) on an array ``t`` of ``dtype``: [..., 4], every operation rounded to ``dtype``."""
    dt = np.dtype(dtype).type
    t = np.asarray(t, dtype)
    A, one = dt(a), dt(1)
    x0 = t + one
    w0 = ((A * x0 - dt(5) * A) * x0 + dt(8) * A) * x0 - dt(4) * A
    w1 = ((A + dt(2)) * t - (A + dt(3))) * t * t + one
    u = one - t
    w2 = ((A + dt(2)) * u - (A + dt(3))) * u * u + one
    x3 = u + one
    w3 = ((A * x3 - dt(5) * A) * x3 + dt(8) * A) * x3 - dt(4) * A
    return np.stack([w0, w1, w2, w3], -1).astype(dtype)


def source_coords(in_size, out_size, dtype=F32):
    """``(floor(src) as int64, t = src - floor(src))`` of every output index, in ``dtype``."""
    dt = np.dtype(dtype).type
    sc = dt(in_size) / dt(out_size)
    src = sc * (np.arange(out_size).astype(dtype) + dt(0.5)) - dt(0.5)
    f = np.floor(src)
    return f.astype(np.int64), (src - f).astype(dtype)


def taps(in_size, out_size, a=-0.75, clamp_hi=None):
    """What the expand body computes per output index: tap indices [out, 4] clamped to [0, in - 1] and f32 weights [out, 4]."""
    f, t = source_coords(in_size, out_size)
    hi = in_size - 1 if clamp_hi is None else clamp_hi
    idx = np.clip(f[:, None] + np.arange(-1, 3)[None, :], 0, max(hi, 0))
    return idx, cubic_weights(t, F32, a)


def coefficients64(in_size, out_size):
    """The same in float64 throughout (coordinates included)."""
    f, t = source_coords(in_size, out_size, np.float64)
    return np.clip(f[:, None] + np.arange(-1, 3)[None, :], 0, in_size - 1), cubic_weights(t, np.float64)


def dense(idx, w, in_size):
    """[out, in]: the weights scattered onto the source indices (clamped taps add up)."""
    m = np.zeros((idx.shape[0], in_size))
    for k in range(4):
        np.add.at(m, (np.arange(idx.shape[0]), idx[:, k]), np.asarray(w[:, k], np.float64))
    return m


def horner_error(t):
    """Running error bound (float64 [..., 4]) of the f32 ``cubic_weights`` at the f32 ``t`` against exact arithmetic at the same t,
    and the largest intermediate: every operation adds ``u |its result|``, a multiplication by x carries the error so far times |x|
    and the factor's own error times the other factor; x0 = t + 1, u = 1 - t and x3 = u + 1 are roundings themselves."""
    t = np.asarray(t, np.float64)
    a = 0.75
    big = np.zeros(t.shape)

    def outer(x, dx):                       # ((A x - 5A) x + 8A) x - 4A
        nonlocal big
        p, e = -a * x, a * dx
        e = e + U * np.abs(p)
        for c in (5 * a, -8 * a, 4 * a):
            q = p + c
            e = e + U * np.abs(q)
            big = np.maximum(big, np.abs(q))
            if c == 4 * a:
                return e
            p = q * x
            e = e * x + np.abs(q) * dx + U * np.abs(p)
            big = np.maximum(big, np.abs(p))

    def inner(x, dx):                       # ((A + 2) x - (A + 3)) x x + 1
        nonlocal big
        p = 1.25 * x
        e = 1.25 * dx + U * np.abs(p)
        q = p - 2.25
        e = e + U * np.abs(q)
        big = np.maximum(big, np.abs(q))
        for _ in range(2):
            p = q * x
            e = e * x + np.abs(q) * dx + U * np.abs(p)
            q = p
        return e + U * np.abs(q + 1.0)

    u = 1.0 - t
    du = U * np.abs(u)
    return np.stack([outer(t + 1.0, U * (t + 1.0)), inner(t, 0.0), inner(u, du), outer(u + 1.0, du + U * (u + 1.0))], -1) * 1.01, big


# ---- oracle and bounds ----------------------------------------------------------------------------------------------------------------
def gather(plane, iy, ix):
    """[out_h, out_w, 4 (rows), 4 (columns)] of the source pixels every output pixel reads."""
    return plane[iy[:, None, :, None], ix[None, :, None, :]]


def resize(plane, out_h, out_w):
    """``dict(want, bound, mag)`` float64 [out_h, out_w] of the bicubic resize of the f32 ``plane`` [h, w]."""
    plane = np.asarray(plane, F32)
    h, w = plane.shape
    if (h, w) == (out_h, out_w):
        want = plane.astype(np.float64)
        return dict(want=want, bound=np.zeros_like(want), mag=np.abs(want))
    (iy, wy), (ix, wx) = taps(h, out_h), taps(w, out_w)
    g = gather(plane.astype(np.float64), iy, ix)
    wy, wx = wy.astype(np.float64)[:, None, :, None], wx.astype(np.float64)[None, :, None, :]
    with np.errstate(invalid='ignore'):
        want = (g * wx * wy).sum((-1, -2))
        mag = (np.abs(g) * np.abs(wx) * np.abs(wy)).sum((-1, -2))
    return dict(want=want, bound=ulp(want) + K_RESIZE * mag, mag=mag)


def word_mean(maps, idxs):
    sel = np.asarray(maps, np.float64)[list(idxs)]
    return dict(want=sel.mean(0), bound=(len(idxs) + 1) * U * np.abs(sel).sum(0) / len(idxs))


def normalize(maps):
    """``dict(want, bound, free)`` of ``maps[:n] / (maps[1:n-1].sum(0) + 1e-6)``: [rows, h, w]."""
    m = np.asarray(maps, np.float64)
    rows = m.shape[0]
    content = m[1:-1]
    s = content.sum(0) + float(EPS_NORM)
    s_abs = np.abs(content).sum(0) + float(EPS_NORM)
    want = m / s
    e_s = max(rows - 2, 0) * U / (1 - rows * U) * s_abs            # |s' - s|
    free = np.broadcast_to(e_s >= np.abs(s) / 2, want.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = e_s / (np.abs(s) - e_s)
        bound = np.where(free, np.inf, np.abs(want) * (rel + (rows + 2 - max(rows - 2, 0)) * U * (1 + rel)))
    return dict(want=want, bound=bound, free=free)


def minmax(res, lo_hi=None):
    """``dict(want, bound, ill, lo, hi, d)`` of the min-max normalisation of ``resize``'s dict."""
    v, b = res['want'], res['bound']
    pick_lo, pick_hi = (np.nanmin, np.nanmax) if lo_hi == 'ignore nan' else (np.min, np.max)
    lo, hi = pick_lo(v), pick_hi(v)
    b_lo = max(lo - pick_lo(v - b), pick_lo(v + b) - lo)
    b_hi = max(pick_hi(v + b) - hi, hi - pick_hi(v - b))
    d = hi - lo + float(EPS_RANGE)
    q = (v - lo) / d
    room = d - b_hi - b_lo
    if room <= 0:
        return dict(want=q, bound=np.full(q.shape, np.inf), ill=True, lo=lo, hi=hi, d=d)
    bound = (b + b_lo + np.abs(q) * (b_hi + b_lo)) / room
    bound = bound + 3 * ulp(np.abs(q) + bound)
    return dict(want=q, bound=bound, ill=bool(np.nanmax(bound) > ILL), lo=lo, hi=hi, d=d)


def expand(plane, out_h, out_w, absolute=False, threshold=None, lo_hi=None, res=None):
    """The oracle of ``expand_word_map``: ``dict(want, bound, ill, ambiguous or None, value, value_bound)``; with a threshold ``want``
    is the 0 / 1 mask and ``ambiguous`` the pixels that may fall on either side."""
    res = resize(plane, out_h, out_w) if res is None else res
    val = dict(want=res['want'], bound=res['bound'], ill=False) if absolute else minmax(res, lo_hi)
    out = dict(want=val['want'], bound=val['bound'], ill=val['ill'], ambiguous=None, value=val['want'], value_bound=val['bound'],
               resize=res)
    if threshold:
        thr = float(F32(threshold))
        out['want'] = (val['want'] > thr).astype(np.float64)
        out['ambiguous'] = (np.abs(val['want'] - thr) <= val['bound']) & (val['bound'] > 0)
    return out


def overlap(a, b):
    """The oracle of ``mask_overlap`` on one pair with a resize: ``dict(lo [3], hi [3], ambiguous)``: each sum's interval."""
    res = resize(a, *b.shape)
    sure = res['want'] - 1.0 > res['bound']
    amb = np.abs(res['want'] - 1.0) <= res['bound']
    b64 = np.asarray(b, np.float64)
    lo = np.array([b64[sure].sum(), sure.sum(), b64.sum()])
    return dict(lo=lo, hi=lo + np.array([b64[amb].sum(), amb.sum(), 0.0]), ambiguous=amb)


def overlap_same_size(a, b):
    """Same sizes, soft values: no resize, no binarisation.  ``dict(want [3], bound [3])``."""
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    waves = -(-a64.size // 64)
    terms = np.array([np.abs(a64 * b64).sum(), np.abs(a64).sum(), np.abs(b64).sum()])
    return dict(want=np.array([(a64 * b64).sum(), a64.sum(), b64.sum()]), bound=terms * (waves + 6) * U)


def overlap_prediction(kind, h, w, seed=0):
    rng = np.random.default_rng([seed, h, w, OVERLAP_KINDS.index(kind)])
    if kind == 'soft':
        return (rng.random((h, w)) * 2.0).astype(F32)
    if kind == 'blocks':            # {0, 2} in blocks of 6 whose edges lie at 6 k - 1: away from the edges the value is 0 or 2, and no
        # edge lies where 64 -> 200 samples half-way between two source rows (rows 4 k - 1 | 4 k), which would give exactly 1
        cells = rng.integers(0, 2, (h // 6 + 2, w // 6 + 2)) * 2.0
        return np.repeat(np.repeat(cells, 6, 0), 6, 1)[1:h + 1, 1:w + 1].astype(F32)
    return planes('levels', 1, h, w, seed)[0] * F32(4.0)


def truth(h, w, seed=0):
    return (np.random.default_rng([seed, h, w, 99]).random((h, w)) > 0.5).astype(F32)


# ---- the kernels in f32 numpy, and their mutants ----------------------------------------------------------------------------------------
def emulate_normalize(maps, drop_eps=False):
    m = np.asarray(maps, F32)
    s = np.zeros(m.shape[1:], F32)
    for t in range(1, m.shape[0] - 1):
        s = s + m[t]
    if not drop_eps:
        s = s + EPS_NORM
    with np.errstate(divide='ignore', invalid='ignore'):
        return m / s


def emulate_word_mean(maps, idxs, distinct=False):
    s = np.zeros(maps.shape[1:], F32)
    for i in idxs:
        s = s + maps[i]
    return s / F32(len(set(idxs)) if distinct else len(idxs))


def emulate_resize(plane, out_h, out_w, swap=False, clamp_short=False, a=-0.75):
    """word_expand[_rect]_kernel's values.  ``swap``: the row pass takes the y weights and the column pass the x weights;
    ``clamp_short``: taps clamped to in - 2; ``a``: the cubic constant."""
    plane = np.asarray(plane, F32)
    h, w = plane.shape
    if (h, w) == (out_h, out_w):
        return plane.copy()
    (iy, wy), (ix, wx) = (taps(n, o, a, n - 2 if clamp_short else None) for n, o in ((h, out_h), (w, out_w)))
    g = gather(plane, iy, ix)
    wr, wc = wx[None, :, None, :], wy[:, None, :]                  # row pass [.., .., 1, 4 columns], column pass [.., 1, 4 rows]
    if swap:
        wr, wc = wy[:, None, None, :], wx[None, :, :]
    p = g * wr
    rows = ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]
    c = rows * wc
    return ((c[..., 0] + c[..., 1]) + c[..., 2]) + c[..., 3]


def _int_order_min_max(v):
    """Minimum and maximum under a plain signed-int compare of the bit patterns (the mutant without ``enc_ordered``)."""
    bits = v.view(np.int32)
    return v[bits.argmin()], v[bits.argmax()]


def emulate_expand(plane, out_h, out_w, absolute=False, threshold=None, whole_waves_only=False, int_order=False, ge=False,
                   drop_eps=False, resized=None, **resize_mutant):
    v = emulate_resize(plane, out_h, out_w, **resize_mutant) if resized is None else resized
    if not absolute:
        flat = v.reshape(-1)
        seen = flat[:flat.size // 64 * 64] if whole_waves_only else flat
        with np.errstate(invalid='ignore'):
            if seen.size == 0:
                lo, hi = F32(np.inf), F32(-np.inf)
            elif int_order:
                lo, hi = _int_order_min_max(seen)
            else:
                lo, hi = np.fmin.reduce(seen), np.fmax.reduce(seen)
            d = (hi - lo) if drop_eps else (hi - lo) + EPS_RANGE
            with np.errstate(divide='ignore'):
                v = (v - lo) / d
    if threshold:
        with np.errstate(invalid='ignore'):
            v = ((v >= F32(threshold)) if ge else (v > F32(threshold))).astype(F32)
    return v


def emulate_overlap(a, b):
    """(sum(a b), sum(a), sum(b)) as float64 of exact integers: the resize leg of mask_overlap_kernel."""
    v = emulate_resize(a, *b.shape)
    va = np.where(v < 1, F32(0), F32(1)).astype(np.float64)
    return np.array([(va * b).sum(), va.sum(), np.asarray(b, np.float64).sum()])


# ---- reporting ------------------------------------------------------------------------------------------------------------------------
def ratio(got, ref, skip=None):
    """Worst ``|got - want| / bound`` over the elements not in ``skip`` (0 / 0 counts as 0; any error against a zero bound as inf)."""
    err = np.abs(np.asarray(got, np.float64) - ref['want'])
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / ref['bound'])
    r = np.where(np.isnan(r), np.inf, r)
    if skip is not None:
        r = np.where(skip, 0.0, r)
    return float(r.max()) if r.size else 0.0


def mask_mismatches(got, ref):
    """``(ambiguous pixels, of them differing, unambiguous pixels differing)`` of a thresholded result."""
    differ = np.asarray(got, np.float64) != ref['want']
    amb = ref['ambiguous']
    return int(amb.sum()), int((differ & amb).sum()), int((differ & ~amb).sum())


# ---- the cases of the GPU file ----------------------------------------------------------------------------------------------------------
def expand_cases():
    """(sizes, kind, absolute, threshold) of every ``expand_word_map`` case."""
    for sizes in SIZE_SETS:
        for kind in EXPAND_KINDS:
            for absolute, threshold in MODES:
                yield sizes, kind, absolute, threshold
    for sizes, kind in EXTRA_CASES:
        for threshold in EXTRA_THRESHOLDS:
            for absolute in (False, True):
                yield sizes, kind, absolute, threshold


def may_be_ill(sizes, kind):
    """The min-max cases that may be ill-conditioned: see the module docstring, "Caps"."""
    return kind == 'constant' or sizes[0] == (1, 1) or sizes[1] == (1, 1)


def check_expand(got, ref, what):
    """Assert one ``expand_word_map`` result [out_h, out_w] against ``expand``'s dict; returns a dict of figures."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref['want'].shape, what
    assert np.isfinite(got).all(), f'{what}: non-finite output'
    if ref['ambiguous'] is None:
        if ref['ill']:
            assert got.min() >= 0.0 and got.max() <= 1.0, f'{what}: ill-conditioned plane outside [0, 1]: {got.min()} .. {got.max()}'
            return dict(ratio=0.0, ill=True)
        r = ratio(got, ref)
        assert r <= 1.0, f'{what}: err / bound {r:.3f}'
        return dict(ratio=r, ill=False)
    assert np.isin(got, (0.0, 1.0)).all(), what
    if ref['ill']:
        return dict(ill=True, ambiguous=0, flipped=0)
    amb, flipped, wrong = mask_mismatches(got, ref)
    assert wrong == 0, f'{what}: {wrong} mask pixels differ away from the threshold'
    return dict(ill=False, ambiguous=amb, flipped=flipped)
