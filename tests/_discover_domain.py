"""Shared by ``test_discover_cpu.py`` and ``test_gpu_discover.py``: the four passes of ``libdaam_discover.so`` (include/daam_discover.h,
DESIGN 3.27) and the whole ``SelfAffinity.discover`` loop as float64 numpy restatements, the error bounds, the mutants that show the
bounds can fail, the case tables, the planted affinities and a numpy stand-in of the library that puts the Python layer under test
without a GPU.  Test-only: the product has no fallback.

Error bounds, all derived from the operations with u = 2^-24 and (1 + 2^-9) for the second-order terms; nothing is fitted to device
output.

``prepare``   The row sum is a chain of c = ceil(N / 256) - 1 + 8 additions per element (a lane's ascending partial sum, then the 8
              levels of the pairwise tree): |s^ - s| <= c u sum|src|.  p = src / s^ adds one division: with kappa = sum|src| / |s|
              (1 for an affinity, whose entries are >= 0), |p^ - p| <= (c kappa + 1) u (1 + 2^-9) |p| + 2^-149.  l = logf(max(p^,
              eps)): max(., eps) is 1-Lipschitz in the logarithm, so l carries p's RELATIVE error as an ABSOLUTE one, plus logf's own
              error.  The HIP math API reference of ROCm (docs/reference/math_api.rst of the HIP documentation, the table of
              single-precision functions; it is not shipped under the ROCm installation directory, only the Doxygen of the runtime
              API is) gives logf a maximum error of 1 ULP; 1 ULP of l is at most 2 u |l|, and at least 2^-149.
``pair_kl``   Against float64 on the same f32 P and L.  A term is t_j = (pa - pb)(la - lb): two subtractions (u each), the product is
              not rounded on its own (fma), and the chain of N fma roundings, j ascending: |D^ - D| <= 1/2 (N + 3) u (1 + 2^-9)
              sum_j |t_j| + 2^-126 (the floor covers the halving and subnormal terms).  Every term is >= 0 when L = log P.
``merge``     cnt - 1 additions and the division: |out^ - out| <= cnt u (1 + 2^-9) sum_r |P_r| / cnt + 2^-149.
``labels``    A resized value is wy0 (wx0 v00 + wx1 v01) + wy1 (wx0 v10 + wx1 v11): 4 products and 3 sums -- on the device the sums are
              fused, and the four weights, each ONE rounding of a ratio of integers, take the roundings the fusing saves; along any
              tap's path at most 6 roundings meet, and the weights sum to 1, so |v^ - v| <= E = 7 u max|props|.  A decision compares
              two such values, so a pixel is held to the float64 argmax when the float64 top-two margin exceeds 2 E, and is left out
              otherwise (at most 1 % of a case).
"""
import ctypes
import math

import numpy as np

import _sweep_domain as S

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
EPS = 2.0 ** -120
LN_EPS = math.log(EPS)
SECOND = 1 + 2.0 ** -9
E_INVALID = -1
THREADS = 256
LOGF_ULPS = 1                                         # HIP math API reference: logf, maximum error 1 ULP


# ---- float64 restatements -------------------------------------------------------------------------------------------------------------
def prepare64(src, eps=EPS):
    """``(P, L)`` float64 of src [R, N]: rows over their sums (zeros where the sum is 0 or not finite), ``log(max(P, eps))``;
    ``eps=None`` is the mutant without the clamp."""
    src = np.asarray(src, F64)
    s = src.sum(axis=1, keepdims=True)
    ok = (s != 0) & np.isfinite(s)
    p = np.where(ok, src / np.where(ok, s, 1), 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        l = np.log(p if eps is None else np.maximum(p, eps))
    return p, l


def sum_chain(n):
    return -(-n // THREADS) - 1 + 8


def prepare_bounds(src):
    """``(bound_P, bound_L)`` [R, N] against ``prepare64`` (module docstring)."""
    src = np.asarray(src, F64)
    p, l = prepare64(src)
    s = src.sum(axis=1, keepdims=True)
    ok = (s != 0) & np.isfinite(s)
    kappa = np.where(ok, np.abs(src).sum(axis=1, keepdims=True) / np.where(ok, np.abs(s), 1), 0.0)
    rel = (sum_chain(src.shape[1]) * kappa + 1) * U * SECOND
    return rel * np.abs(p) + 2.0 ** -149, rel + LOGF_ULPS * 2 * U * np.abs(l) + 2.0 ** -149


def pair_kl64(pa, la, pb, lb, chunk=64):
    """float64 [A, B] on the values given: 1/2 sum_j (pa - pb)(la - lb)."""
    pa, la, pb, lb = (np.asarray(x, F64) for x in (pa, la, pb, lb))
    out = np.zeros((pa.shape[0], pb.shape[0]))
    for a in range(0, pa.shape[0], chunk):
        out[a:a + chunk] = 0.5 * np.einsum('abj,abj->ab', pa[a:a + chunk, None] - pb[None], la[a:a + chunk, None] - lb[None])
    return out


def pair_kl_bound(pa, la, pb, lb, chunk=64):
    pa, la, pb, lb = (np.asarray(x, F64) for x in (pa, la, pb, lb))
    out = np.zeros((pa.shape[0], pb.shape[0]))
    for a in range(0, pa.shape[0], chunk):
        out[a:a + chunk] = np.abs((pa[a:a + chunk, None] - pb[None]) * (la[a:a + chunk, None] - lb[None])).sum(axis=2)
    return 0.5 * (pa.shape[1] + 3) * U * SECOND * out + 2.0 ** -126


def merge64(p, member):
    """``(out [K, N] float64, cnt [K])``."""
    p, m = np.asarray(p, F64), np.asarray(member) != 0
    cnt = m.sum(axis=1)
    return (m.astype(F64) @ p) / np.maximum(cnt, 1)[:, None], cnt.astype(np.int32)


def merge_bound(p, member):
    m = np.asarray(member) != 0
    cnt = m.sum(axis=1)
    return cnt[:, None] * U * SECOND * (m.astype(F64) @ np.abs(np.asarray(p, F64))) / np.maximum(cnt, 1)[:, None] + 2.0 ** -149


def taps(o, n_in, n_out, align_corners=False):
    """``(i0, i1, w0, w1)`` float64 arrays for the output indices ``o`` along an axis: F.interpolate's bilinear taps."""
    o = np.asarray(o, F64)
    if align_corners:
        pos = o * ((n_in - 1) / (n_out - 1)) if n_out > 1 else 0 * o
    else:
        pos = np.maximum(((2 * o + 1) * n_in - n_out) / (2 * n_out), 0.0)
    i0 = np.minimum(np.floor(pos).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = pos - i0
    return i0, i1, 1 - w1, w1


def resize64(props, out_h, out_w, align_corners=False):
    """float64 [K, out_h, out_w]: the bilinear resize of props [K, h, w]."""
    props = np.asarray(props, F64)
    y0, y1, wy0, wy1 = taps(np.arange(out_h), props.shape[1], out_h, align_corners)
    x0, x1, wx0, wx1 = taps(np.arange(out_w), props.shape[2], out_w, align_corners)
    top = props[:, y0][:, :, x0] * wx0 + props[:, y0][:, :, x1] * wx1
    bot = props[:, y1][:, :, x0] * wx0 + props[:, y1][:, :, x1] * wx1
    return top * wy0[None, :, None] + bot * wy1[None, :, None]


def labels64(props, out_h, out_w, align_corners=False, highest=False):
    """``(labels [out_h, out_w], values, decided)``: the float64 argmax (lowest index on a tie; ``highest`` is the mutant), the winner's
    value, and where the top-two margin exceeds twice the bilinear error bound (every pixel with one proposal)."""
    v = resize64(props, out_h, out_w, align_corners)
    lab = v.shape[0] - 1 - np.argmax(v[::-1], axis=0) if highest else np.argmax(v, axis=0)
    if v.shape[0] == 1:
        return lab.astype(np.uint8), v[0], np.ones((out_h, out_w), bool)
    top2 = np.partition(v, -2, axis=0)[-2:]
    return lab.astype(np.uint8), v.max(axis=0), (top2[1] - top2[0]) > 2 * labels_bound(props)


def labels_bound(props):
    return 7 * U * float(np.abs(np.asarray(props, F64)).max())


def anchors_of(grid, anchors):
    h, w = grid
    rows, cols = (anchors, anchors) if isinstance(anchors, int) else anchors
    ys = [min(int(math.floor((r + 0.5) * h / rows)), h - 1) for r in range(rows)]
    xs = [min(int(math.floor((c + 0.5) * w / cols)), w - 1) for c in range(cols)]
    return [y * w + x for y in ys for x in xs]


def greedy(d, threshold):
    used, groups = [False] * len(d), []
    for i in range(len(d)):
        if used[i]:
            continue
        group = [i] + [j for j in range(len(d)) if j != i and not used[j] and d[i][j] < threshold]
        for j in group:
            used[j] = True
        groups.append(group)
    return groups


def discover64(sums, grid, anchors=16, threshold=1.1, iterations=3, size=None, matrices=None):
    """``(labels [H, W], proposals float64 [K, h, w])`` of the whole loop in float64.  ``matrices``: a list that receives every D."""
    h, w = grid
    p, l = prepare64(sums)
    idx = anchors_of(grid, anchors)
    d = pair_kl64(p[idx], l[idx], p, l)
    member = d < threshold
    member[np.arange(len(idx)), idx] = True
    props, _ = merge64(p, member)
    if matrices is not None:
        matrices.append(d)
    for _ in range(iterations - 1):
        pp, lp = prepare64(props)
        d = pair_kl64(pp, lp, pp, lp)
        if matrices is not None:
            matrices.append(d)
        groups = greedy(d, threshold)
        member = np.zeros((len(groups), len(props)), bool)
        for k, g in enumerate(groups):
            member[k, g] = True
        props, _ = merge64(pp, member)
    out_h, out_w = (h, w) if size is None else size
    props = props.reshape(-1, h, w)
    return labels64(props, out_h, out_w)[0], props


def same_partition(a, b):
    """Two label maps describe the same partition, up to a permutation of the labels."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len({x for x, _ in pairs}) == len({y for _, y in pairs})


# ---- planted affinities ----------------------------------------------------------------------------------------------------------------
PLANTED_GRIDS = ((4, 4), (5, 7), (8, 8), (9, 13), (16, 16))
PLANTED_SEGMENTS = (2, 3, 5)
PLANTED = [(s, g) for s in PLANTED_SEGMENTS for g in PLANTED_GRIDS]
DELTA = 0.1
THRESHOLD = 1.1


def planted(segments, grid, seed=0):
    """``(sums f32 [P, P], truth [h, w])``: row i is (1 - DELTA) uniform on its own segment plus DELTA uniform on all cells, times a
    per-row scale, with 1 % of seeded noise.  Segments are runs of the row-major cell order.  Within a segment D is about 1e-4, across
    segments about (1 - DELTA) ln(1 + (1 - DELTA) S / DELTA) >= 2.6."""
    h, w = grid
    cells = h * w
    rng = np.random.default_rng(1000 * segments + cells + seed)
    truth = (np.arange(cells) * segments) // cells
    own = (truth[:, None] == truth[None, :]).astype(F64)
    rows = (1 - DELTA) * own / own.sum(axis=1, keepdims=True) + DELTA / cells
    rows = rows * rng.uniform(1.0, 40.0, (cells, 1)) * (1 + 0.01 * rng.uniform(-1, 1, (cells, cells)))
    return rows.astype(F32), truth.reshape(h, w)


# ---- case tables -----------------------------------------------------------------------------------------------------------------------
# prepare: (R, N, kind).  R, N in {1, 5, 63, 65, 130, 257}: a lane has one cell or several, the tree has empty leaves or none.
PREPARE_KINDS = ('plain', 'strided', 'zero_row', 'one_cell', 'magnitudes')
PREPARE_CASES = [(1, 1, 'plain'), (5, 257, 'strided'), (63, 65, 'zero_row'), (65, 63, 'one_cell'), (130, 5, 'magnitudes'),
                 (257, 130, 'plain'), (5, 1, 'zero_row'), (1, 257, 'magnitudes'), (130, 130, 'strided'), (63, 5, 'one_cell')]


def prepare_inputs(case):
    """``(buffer f32 [R, stride], stride)``; the source is ``buffer[:, :N]``."""
    r, n, kind = case
    rng = np.random.default_rng(r * 1000 + n)
    stride = n + 3 if kind == 'strided' else n
    buf = rng.uniform(0.05, 1.0, (r, stride))
    if kind == 'magnitudes':
        buf *= 2.0 ** rng.integers(-30, 31, (r, 1))
    if kind == 'zero_row':
        buf[r // 2, :n] = 0
    if kind == 'one_cell':
        buf[:, :n] = 0
        buf[np.arange(r), rng.integers(0, n, r)] = rng.uniform(0.5, 2.0, r)
    return buf.astype(F32), stride


# pair_kl: (A, B, N, regime).  A tile is 64 x 64 and a chunk 32 cells; N a multiple of 4 takes the float4 loads, any other N the scalar
# ones.  'self' passes Pa as Pb (A == B).
PAIR_REGIMES = ('smooth', 'near', 'disjoint', 'self')
PAIR_CASES = [(1, 1, 1, 'smooth'), (3, 63, 7, 'near'), (63, 3, 64, 'disjoint'), (65, 65, 65, 'self'), (130, 1, 257, 'smooth'),
              (1, 130, 1024, 'near'), (63, 65, 1024, 'disjoint'), (130, 130, 64, 'self'), (3, 3, 257, 'self'), (65, 130, 7, 'smooth'),
              (130, 63, 65, 'near'), (65, 3, 257, 'disjoint'), (63, 63, 1, 'self'), (3, 65, 64, 'smooth'), (65, 63, 64, 'near'),
              (3, 130, 1024, 'disjoint'), (65, 65, 1024, 'self'), (130, 65, 7, 'disjoint')]


def case_id(c):
    return '-'.join(str(x) if not isinstance(x, tuple) else 'x'.join(map(str, x)) for x in c)


def _rows(rng, rows, n, regime, parity):
    if regime == 'near':                              # one base row for both sides (seeded by N alone), 0.1 % of noise per row
        base = np.random.default_rng(n).uniform(0.5, 1.5, (1, n))
        src = base * (1 + 1e-3 * rng.uniform(-1, 1, (rows, n)))
    else:
        src = rng.uniform(0.1, 1.1, (rows, n))
    if regime == 'disjoint' and n > 1:
        src[:, (np.arange(n) + parity) % 2 == 1] = 0
    return src


def pair_inputs(case):
    """``(Pa, La, Pb, Lb)`` f32: probability rows and their logarithms as f32 values (what ``prepare`` gives in exact arithmetic,
    rounded once); with 'self' the b side IS the a side."""
    a, b, n, regime = case
    rng = np.random.default_rng(a * 10000 + b * 100 + n)
    pa, la = (x.astype(F32) for x in prepare64(_rows(rng, a, n, regime, 0)))
    if regime == 'self':
        return pa, la, pa, la
    pb, lb = (x.astype(F32) for x in prepare64(_rows(rng, b, n, regime, 1)))
    return pa, la, pb, lb


# merge: (K, R, N).
MERGE_CASES = [(k, r, n) for (k, r), n in zip([(k, r) for k in (1, 3, 33) for r in (1, 64, 257)], (5, 130, 257, 1, 65, 300, 63, 256, 7))]


def merge_inputs(case):
    """``(P f32 [R, N], member u8 [K, R])``: group 0 empty (when K > 1), group 1 full, group 2 a single member, the rest random; bytes
    that are set are any non-zero value."""
    k, r, n = case
    rng = np.random.default_rng(k * 1000 + r + n)
    p = rng.uniform(0, 1, (r, n)).astype(F32)
    member = (rng.uniform(0, 1, (k, r)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (k, r)).astype(np.uint8)
    if k > 1:
        member[0] = 0
        member[1] = 1
    if k > 2:
        member[2] = 0
        member[2, r // 2] = 255
    return p, member


# labels: (K, (h, w), (out_h, out_w), kind).
LABEL_KINDS = ('plateaus', 'smooth')
_OUTS = ('same', 'x2', (37, 53), (128, 128))
LABEL_CASES = [(k, g, (g if o == 'same' else (2 * g[0], 2 * g[1]) if o == 'x2' else o), LABEL_KINDS[(ki + gi + oi) % 2])
               for ki, k in enumerate((1, 2, 7, 255)) for gi, g in enumerate(((4, 4), (5, 7), (16, 16))) for oi, o in enumerate(_OUTS)
               if (ki + gi + oi) % 2 == 0 or k == 7]


def label_inputs(case):
    """props f32 [K, h, w]: 'plateaus' -- proposal k is 1 + k / 64 on the cells of its run of the row-major order and a small seeded
    ground elsewhere; 'smooth' -- seeded uniform values."""
    k, (h, w), _, kind = case
    rng = np.random.default_rng(k * 100 + h * w)
    if kind == 'smooth':
        return rng.uniform(0, 1, (k, h, w)).astype(F32)
    owner = (np.arange(h * w) * min(k, h * w)) // (h * w)
    props = rng.uniform(0, 0.05, (k, h * w))
    props[owner, np.arange(h * w)] = 1 + owner / 64
    return props.reshape(k, h, w).astype(F32)


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
def pair_kl_mutant(pa, la, pb, lb, mutant):
    pa, la, pb, lb = (np.asarray(x, F64) for x in (pa, la, pb, lb))
    if mutant == 'one_sided':
        return np.einsum('aj,abj->ab', pa, la[:, None] - lb[None])
    if mutant == 'no_half':
        return 2 * pair_kl64(pa, la, pb, lb)
    if mutant == 'neighbour_L':
        return pair_kl64(pa, np.roll(la, -1, axis=0), pb, lb)
    if mutant == 'past_N':                             # three cells past the row's end: the next row's first ones (zeros after the last)
        ext = lambda x: np.concatenate([x.reshape(-1), np.zeros(3)])[np.arange(x.shape[0])[:, None] * x.shape[1] + np.arange(x.shape[1] + 3)]
        return pair_kl64(ext(pa), ext(la), ext(pb), ext(lb))
    raise ValueError(mutant)


def merge_mutant(p, member, mutant):
    p, m = np.asarray(p, F64), np.asarray(member) != 0
    if mutant == 'transposed':                         # the bytes of [K][R] read as [R][K]
        m = m.reshape(-1).reshape(m.shape[1], m.shape[0]).T
        return (m.astype(F64) @ p) / np.maximum(m.sum(axis=1), 1)[:, None]
    if mutant == 'mean_over_R':
        return (m.astype(F64) @ p) / p.shape[0]
    raise ValueError(mutant)


# ---- a numpy stand-in of the library ---------------------------------------------------------------------------------------------------
class FakeDiscoverLib:
    """The four entry points in numpy (float64 arithmetic rounded to f32) on CPU tensors' memory, held to the header's limits; ``calls``
    records ``(name, shape...)``."""

    def __init__(self):
        self.calls = []

    def daam_discover_abi_version(self):
        return 1

    def daam_discover_last_error(self):
        return b''

    def daam_discover_prepare(self, src, stride, r, n, p, l, stream):
        assert src and p and l and 1 <= r <= 16384 and 1 <= n <= 16384 and stride >= n
        self.calls.append(('prepare', r, n, stride))
        rows = S._array(src, ctypes.c_float, (r - 1) * stride + n)
        rows = np.stack([rows[i * stride:i * stride + n] for i in range(r)])
        p64, l64 = prepare64(rows)
        S._array(p, ctypes.c_float, r * n)[:] = p64.astype(F32).reshape(-1)
        S._array(l, ctypes.c_float, r * n)[:] = np.log(np.maximum(p64.astype(F32).astype(F64), EPS)).astype(F32).reshape(-1)
        return 0

    def daam_discover_pair_kl(self, pa, la, a, pb, lb, b, n, d, stream):
        assert pa and la and pb and lb and d and 1 <= a <= 16384 and 1 <= b <= 16384 and 1 <= n <= 16384
        self.calls.append(('pair_kl', a, b, n))
        get = lambda ptr, rows: S._array(ptr, ctypes.c_float, rows * n).reshape(rows, n).copy()
        S._array(d, ctypes.c_float, a * b)[:] = pair_kl64(get(pa, a), get(la, a), get(pb, b), get(lb, b)).astype(F32).reshape(-1)
        return 0

    def daam_discover_merge(self, p, r, n, member, k, out, cnt, stream):
        assert p and member and out and cnt and 1 <= r <= 16384 and 1 <= n <= 16384 and 1 <= k <= 1024
        self.calls.append(('merge', r, n, k))
        o, c = merge64(S._array(p, ctypes.c_float, r * n).reshape(r, n), S._array(member, ctypes.c_uint8, k * r).reshape(k, r))
        S._array(out, ctypes.c_float, k * n)[:] = o.astype(F32).reshape(-1)
        S._array(cnt, ctypes.c_int32, k)[:] = c
        return 0

    def daam_discover_labels(self, props, k, h, w, out_h, out_w, labels, values, stream):
        assert props and labels and 1 <= k <= 255 and 1 <= h <= 128 and 1 <= w <= 128 and 1 <= out_h <= 2048 and 1 <= out_w <= 2048
        self.calls.append(('labels', k, h, w, out_h, out_w))
        lab, val, _ = labels64(S._array(props, ctypes.c_float, k * h * w).reshape(k, h, w), out_h, out_w)
        S._array(labels, ctypes.c_uint8, out_h * out_w)[:] = lab.reshape(-1)
        if values:
            S._array(values, ctypes.c_float, out_h * out_w)[:] = val.astype(F32).reshape(-1)
        return 0


def install(setattr_):
    """``_sweep_domain.install`` (CPU tensors pass for device tensors) plus a ``FakeDiscoverLib`` under ``daam_amd.engine``; ``loads``
    counts the calls of ``load_discover``.  Returns ``(engine module, lib, loads)``."""
    E, _ = S.install(setattr_)
    lib, loads = FakeDiscoverLib(), []

    def load():
        loads.append(1)
        return lib
    setattr_(E.nat, 'load_discover', load)
    setattr_(E, '_check_discover_device', lambda t, like: None)
    return E, lib, loads
