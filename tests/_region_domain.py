"""Shared by ``test_region_scores_cpu.py`` and ``test_gpu_region_scores.py``: masks and planes for ``daam_region_scores``
(daam_amd/csrc/daam_region_scores.hip), a float64 oracle, the per-score bound, and an f32 numpy emulation of the kernels in their
operation order whose switches are the mutants the CPU file proves the cases catch.

Definition.  ``score[g, m, t] = sum over the set pixels (y, x) of mask m of E_t[y, x]``, ``E_t`` = the bicubic expansion of
``maps[g, t]`` that ``word_expand[_rect]_kernel`` writes under ``absolute``; by linearity ``= sum_ij F[m, i, j] maps[g, t, i, j]`` with the
footprint ``F[m] = Ay^T mask_m Ax``, ``Ay`` [H, h] / ``Ax`` [W, w] the resize's weights scattered onto their (border-clamped) taps.

Oracle.  The coefficients are computed in f32 in the kernels' order (``_epilogue_domain.taps``: they are inputs of the comparison, as in
the epilogue domain); everything after them is float64: ``F64 = Ay^T mask Ax``, ``want = sum F64 v``, and ``S = sum F_abs |v|`` with
``F_abs`` built from ``|wy| |wx|``.  At identity sizes ``Ay`` and ``Ax`` are identities.

Bound.  ``|got - want| <= ulp(want) + g_K S``, ``g_K = K u / (1 - K u)``, ``u = 2^-24``, K = the roundings on the longest path of one
term ``wy wx v`` through the kernels (every product and sum is rounded on its own, contraction is off):

  fold      3 + 3   the weights of clamped taps are added onto the edge cell, per axis: at most three additions
  x pass    Lx      thread (row, cell j) adds the weights of the row's set pixels that reach j, one chain in ascending x:
                    Lx = the most pixels of a row that reach one cell (about 4 W / w; the whole row when w <= 4)
  y pass    1 + Ly  weight x row sum, then one chain over the band's rows in ascending y: Ly = min(rows of a band (<= 32), the
                    most rows that reach one cell row)
  combine   Nb      the partials of the bands that reach a cell row, ascending: Nb = the most bands any cell row is reached from
  dot       1 + ceil(h w / 256) + 8     the product, a lane's chain over its cells, six butterfly steps, (a + b) + (c + d) over four waves

``roundings(geom)`` computes K from the tables; the CPU file asserts ``K u <= 2^-14`` on every case of the GPU file (the largest is
the 64^2 -> 1024^2 case: Lx = 88, Ly = 32, Nb = 3, dot 25: K = 155, K u = 2^-16.7).

``emulate`` follows the kernels: the folded tables, the integer cell ranges (``cell_range``: a superset of the pixels that reach a cell,
so a range that is too narrow shows as an error), the bands and their windows of cell rows, the band order of the combine, the lane
chains and trees of the dot."""
import numpy as np

from _epilogue_domain import F32, U, cubic_weights, dense, planes, source_coords, taps, ulp

MAX_MASKS = 32
BAND_ROWS, TILE_PIXELS, THREADS = 32, 32768, 256
CAP = 2.0 ** -14

# map -> mask sizes (the issue's table); the last one runs with three masks only
SIZE_SETS = [((64, 64), (128, 128)), ((64, 64), (200, 333)), ((16, 24), (37, 53)), ((48, 48), (32, 32)), ((12, 20), (12, 20)),
             ((1, 1), (5, 7)), ((2, 2), (9, 9)), ((8, 8), (1, 1)), ((128, 128), (256, 256)), ((52, 76), (208, 304)),
             ((64, 64), (1024, 1024))]
LONG = ((64, 64), (1024, 1024))
MASK_KINDS = ('random', 'all_set', 'all_clear', 'corner_tl', 'corner_tr', 'corner_bl', 'corner_br', 'row', 'column', 'checker',
              'blocks', 'random255', 'random2')
PLANE_KINDS = ('real', 'signed', 'levels', 'tiny')
ROWS = 5
ZERO_ROW, BIG_ROW = 3, 2


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def mask(kind, H, W, seed=0):
    """uint8 [H, W] of ``kind``."""
    rnd = (np.random.default_rng([seed, H, W, 40]).random((H, W)) < 0.4)
    m = np.zeros((H, W), np.uint8)
    if kind == 'random':
        m[rnd] = 1
    elif kind == 'random255':
        m[rnd] = 255
    elif kind == 'random2':
        m[rnd] = 2
    elif kind == 'all_set':
        m[:] = 1
    elif kind == 'all_clear':
        pass
    elif kind.startswith('corner_'):
        m[0 if kind[7] == 't' else H - 1, 0 if kind[8] == 'l' else W - 1] = 1
    elif kind == 'row':
        m[(seed * 7 + H // 3) % H, :] = 1
    elif kind == 'column':
        m[:, (seed * 5 + 2 * W // 3) % W] = 1
    elif kind == 'checker':
        yy, xx = np.mgrid[0:H, 0:W]
        m[(yy + xx) % 2 == 0] = 1
    elif kind == 'blocks':
        cells = np.random.default_rng([seed, H, W, 22]).integers(0, 2, ((H + 1) // 2, (W + 1) // 2))
        m[:] = np.repeat(np.repeat(cells, 2, 0), 2, 1)[:H, :W]
    else:
        raise ValueError(kind)
    return m


def stack_kinds(n, first=0):
    return [MASK_KINDS[(first + i) % len(MASK_KINDS)] for i in range(n)]


def mask_stack(H, W, n, first=0):
    """uint8 [n, H, W]: the kinds in turn from ``first`` on; a kind that comes round again gets another seed.  With n = 32 and
    first = 0 the last mask is 'corner_br': the very last byte of the stack is set."""
    return np.stack([mask(k, H, W, seed=i // len(MASK_KINDS)) for i, k in enumerate(stack_kinds(n, first))])


def map_sets(h, w):
    """f32 [5, ROWS, h, w]: one set per plane kind, and a set whose row ZERO_ROW is exactly zero beside a row of 2^20."""
    sets = [planes(kind, ROWS, h, w) for kind in PLANE_KINDS]
    last = planes('real', ROWS, h, w, seed=1)
    last[BIG_ROW] = F32(2.0 ** 20) * (F32(1.0) + planes('plain', 1, h, w, seed=2)[0])
    last[ZERO_ROW] = 0.0
    return np.stack(sets + [last])


# ---- geometry and tables: what the host and region_tables_kernel compute ---------------------------------------------------------------
def geometry(H, W, h, w):
    band = 1 if W >= TILE_PIXELS else min(TILE_PIXELS // W, BAND_ROWS)
    return dict(H=H, W=W, h=h, w=w, band=band, n_bands=-(-H // band), win=min(h, -(-(h * band) // H) + 6),
                margin_y=1 + (H >> 20), margin_x=1 + (W >> 20))


def cell_range(j, N, n, margin):
    lo = 0 if j == 0 else min(max((2 * j - 3) * N // (2 * n) - 1 - margin, 0), N)
    hi = N if j == n - 1 else min(-(-(2 * j + 5) * N // (2 * n)) + margin, N)
    return lo, hi


def tables(n_in, n_out, identity, shift=0, fold_inside=False, sc_from=None):
    """``(base [out], fold f32 [out, 4])``: the first cell an output index reaches and its four folded weights.  Mutants: ``shift``
    moves the taps, ``fold_inside`` puts a clamped tap's weight on the cell next to the edge, ``sc_from`` = (in, out) takes the
    scale of another axis."""
    if identity:
        fold = np.zeros((n_out, 4), F32)
        fold[:, 0] = 1
        return np.arange(n_out), fold
    if sc_from is None:
        _, wt = taps(n_in, n_out)
        f, _ = source_coords(n_in, n_out)
    else:
        sc = F32(sc_from[0]) / F32(sc_from[1])
        src = sc * (np.arange(n_out).astype(F32) + F32(0.5)) - F32(0.5)
        f = np.floor(src).astype(np.int64)
        wt = cubic_weights((src - np.floor(src)).astype(F32))
    unclamped = f[:, None] + np.arange(-1, 3)[None, :] + shift
    cells = np.clip(unclamped, 0, n_in - 1)
    if fold_inside and n_in > 2:
        cells = np.where(unclamped < 0, 1, np.where(unclamped > n_in - 1, n_in - 2, cells))
    base = np.clip(f - 1 + shift, 0, n_in - 1)
    if fold_inside:
        base = cells.min(1)
    fold = np.zeros((n_out, 4), F32)
    for a in range(4):
        k = cells[:, a] - base
        assert (k >= 0).all() and (k < 4).all()
        fold[np.arange(n_out), k] = fold[np.arange(n_out), k] + wt[:, a]
    return base, fold


def _dense32(base, fold, n_in, ranges=None):
    """f32 [out, in]: the folded weights on their cells; outside ``ranges[j]`` (the pass's cell range) a pixel is not looked at."""
    n_out = base.shape[0]
    g = np.zeros((n_out, n_in), F32)
    for k in range(4):
        ok = base + k < n_in
        g[np.arange(n_out)[ok], (base + k)[ok]] = fold[ok, k]
    if ranges is not None:
        o = np.arange(n_out)[:, None]
        g = np.where((o >= ranges[:, 0][None, :]) & (o < ranges[:, 1][None, :]), g, F32(0))
    return g


def _reach(base, n_in):
    """bool [out, in]: output index o reaches cell j (base <= j <= base + 3)."""
    j = np.arange(n_in)[None, :]
    return (base[:, None] <= j) & (j <= base[:, None] + 3)


def roundings(geom):
    """K of the module docstring for one geometry."""
    H, W, h, w = geom['H'], geom['W'], geom['h'], geom['w']
    ident = (H, W) == (h, w)
    by, _ = tables(h, H, ident)
    bx, _ = tables(w, W, ident)
    lx = int(_reach(bx, w).sum(0).max())
    ry = _reach(by, h)
    ly = min(geom['band'], int(ry.sum(0).max()))
    bands = np.arange(H) // geom['band']
    nb = max(len(set(bands[ry[:, i]])) for i in range(h))
    parts = dict(fold=6, x=lx, y=1 + ly, combine=nb, dot=1 + -(-(h * w) // THREADS) + 8)
    return sum(parts.values()), parts


# ---- oracle ---------------------------------------------------------------------------------------------------------------------------
def footprint64(masks, h, w, set_rule=None):
    """``(F64, F_abs)`` float64 [M, h, w] of uint8 masks [M, H, W]."""
    M, H, W = masks.shape
    if (H, W) == (h, w):
        ay = ay_abs = np.eye(H)
        ax = ax_abs = np.eye(W)
    else:
        (iy, wy), (ix, wx) = taps(h, H), taps(w, W)
        ay, ax = dense(iy, wy, h), dense(ix, wx, w)
        ay_abs, ax_abs = dense(iy, np.abs(wy), h), dense(ix, np.abs(wx), w)
    bits = (masks != 0).astype(np.float64)
    return ay.T[None] @ bits @ ax[None], ay_abs.T[None] @ bits @ ax_abs[None]


def oracle(masks, maps, h, w):
    """``dict(want, mag, bound [G, M, rows], area [M], F64, F_abs, K)`` for masks [M, H, W] and maps [G, rows, h, w]."""
    f64, f_abs = footprint64(masks, h, w)
    v = np.asarray(maps, np.float64)
    want = np.einsum('mij,gtij->gmt', f64, v)
    mag = np.einsum('mij,gtij->gmt', f_abs, np.abs(v))
    K, _ = roundings(geometry(masks.shape[1], masks.shape[2], h, w))
    return dict(want=want, mag=mag, bound=ulp(want) + K * U / (1 - K * U) * mag, area=(masks != 0).sum((1, 2)), F64=f64, F_abs=f_abs, K=K)


def worst(got, ref):
    """Worst ``|got - want| / bound`` (0 / 0 = 0, an error against a zero bound = inf)."""
    err = np.abs(np.asarray(got, np.float64) - ref['want'])
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / ref['bound'])
    return float(np.where(np.isnan(r), np.inf, r).max())


# ---- the kernels in f32 numpy, and their mutants ------------------------------------------------------------------------------------
MUTANTS = ('tap_shift', 'fold_inside', 'drop_last_band', 'gt_one', 'transposed', 'wrong_sc')


def emulate_footprint(masks, h, w, mutant=None):
    """f32 [M, h, w] and the integer areas: region_tables_kernel, region_footprint_kernel and region_combine_kernel."""
    M, H, W = masks.shape
    g = geometry(H, W, h, w)
    ident = (H, W) == (h, w)
    extra = dict(shift=1) if mutant == 'tap_shift' else dict(fold_inside=True) if mutant == 'fold_inside' else {}
    by, fy = tables(h, H, ident)
    bx, fx = tables(w, W, ident, sc_from=(h, H) if mutant == 'wrong_sc' and not ident else None, **extra)
    rx = np.array([cell_range(j, W, w, g['margin_x']) for j in range(w)])
    gx = _dense32(bx, fx, w, rx)                             # [W, w]
    gy = _dense32(by, fy, h)                                 # [H, h]
    bits = (masks > 1) if mutant == 'gt_one' else (masks != 0)
    setf = bits.astype(F32)
    # x pass: one chain per (row, cell) in ascending x; an unset pixel and a pixel that does not reach the cell add nothing
    rows = np.zeros((M, H, w), F32)
    for x in range(W):
        rows = rows + setf[:, :, x, None] * gx[x][None, None, :]
    # y pass per band, in a window of cell rows; then the bands in ascending order, each cell row from the bands of its range
    out = np.zeros((M, h, w), F32)
    ry = np.array([cell_range(i, H, h, g['margin_y']) for i in range(h)])
    n_bands = g['n_bands'] - (1 if mutant == 'drop_last_band' else 0)
    for b in range(n_bands):
        y0, y1 = b * g['band'], min((b + 1) * g['band'], H)
        part = np.zeros((M, h, w), F32)
        for y in range(y0, y1):
            sel = np.arange(by[y], min(by[y] + 4, h))
            part[:, sel] = part[:, sel] + gy[y, sel][None, :, None] * rows[:, y][:, None, :]
        i = np.arange(h)
        seen = (i >= by[y0]) & (i < by[y0] + g['win']) & (ry[:, 0] // g['band'] <= b) & (b <= (ry[:, 1] - 1) // g['band']) & (ry[:, 0] < ry[:, 1])
        out[:, seen] = out[:, seen] + part[:, seen]
    if mutant == 'transposed':
        out = np.ascontiguousarray(out.transpose(0, 2, 1)).reshape(M, h, w)
    return out, bits.sum((1, 2))


def emulate_dots(foot, maps):
    """f32 [G, M, rows]: region_dot_kernel."""
    M = foot.shape[0]
    G, rows = maps.shape[:2]
    cells = foot[0].size
    n = -(-cells // THREADS)
    f = np.zeros((M, n * THREADS), F32)
    f[:, :cells] = foot.reshape(M, cells)
    v = np.zeros((G, rows, n * THREADS), F32)
    v[:, :, :cells] = np.asarray(maps, F32).reshape(G, rows, cells)
    lane = np.zeros((G, M, rows, THREADS), F32)
    for q in range(n):
        s = slice(q * THREADS, (q + 1) * THREADS)
        lane = lane + f[None, :, None, s] * v[:, None, :, s]
    a = lane.reshape(G, M, rows, THREADS // 64, 64)
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        a = a + a[..., idx ^ off]
    a = a[..., 0]
    return (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])


def emulate(masks, maps, h, w, mutant=None):
    foot, area = emulate_footprint(masks, h, w, mutant)
    return emulate_dots(foot, maps), area, foot


# ---- the cases of the GPU file -----------------------------------------------------------------------------------------------------
def cases():
    """``(sizes, M, first kind)`` of every bound case: M = 32, 3 and 1 on every size set but the long one (M = 3)."""
    for sizes in SIZE_SETS:
        if sizes == LONG:
            yield sizes, 3, 0                       # random, all set, all clear
            continue
        yield sizes, 32, 0
        yield sizes, 3, 6                           # the last corner, one row, one column
        yield sizes, 1, 9                           # the checkerboard
