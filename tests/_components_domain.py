"""Shared by ``test_components_cpu.py`` and ``test_gpu_components.py``: the masks of the cases of ``daam_mask_components``
(include/daam_components.h), a numpy union-find labeller over row runs (the reference: 4- and 8-connectivity, what the
call returns as numpy arrays), a breadth-first labeller to hold it against, the kernels' union rules restated pixel by pixel, and a
numpy stand-in of ``libdaam_components`` that puts the Python layer under test without a GPU.  Test-only: the product has no
fallback."""
import ctypes
from collections import deque

import numpy as np

import _epilogue_domain as D
import _locate_domain as L
import _sweep_domain as S

TILE = (32, 256)                            # rows x columns of a workgroup's tile (daam_components.hip)
SEAMS = (67, 531)                           # three tile rows and three tile columns, partial tiles on both edges
BYTES = np.array([1, 2, 128, 255], np.uint8)


# ---- masks -------------------------------------------------------------------------------------------------------------------------------
def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy + xx) % 2 == 0).astype(np.uint8)


def spiral(h, w):
    """A one-pixel-wide path that winds inwards from (0, 0), one clear pixel between its turns: one component, long parent chains."""
    m = np.zeros((h, w), np.uint8)
    inside = lambda y, x: 0 <= y < h and 0 <= x < w
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    turns = 0
    while turns < 2:
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(ny, nx) and not m[ny, nx] and not (inside(fy, fx) and m[fy, fx]):
            y, x = ny, nx
            m[y, x] = 1
            turns = 0
        else:
            dy, dx = dx, -dy
            turns += 1
    return m


def comb(h, w, spine_row=None):
    """Teeth in every second column over the whole height, joined only by a spine (default: the last row): every tooth crosses
    every horizontal seam, and the teeth of one tile meet only in the tile row that holds the spine."""
    m = np.zeros((h, w), np.uint8)
    m[:, ::2] = 1
    m[h - 1 if spine_row is None else spine_row, :] = 1
    return m


def u_shape(h, w):
    """Two arms that lie in the first tile (the right one starts higher, so ITS top is the lower index) and join only in the tile
    below; a separate pixel in a corner."""
    m = np.zeros((h, w), np.uint8)
    m[5:41, 10] = 1
    m[3:41, 200] = 1
    m[40, 10:201] = 1
    m[h - 1, w - 1] = 1
    return m


def ring_and_blob(h, w):
    m = np.zeros((h, w), np.uint8)
    m[5, 5:w - 20] = m[h - 6, 5:w - 20] = 1
    m[5:h - 5, 5] = m[5:h - 5, w - 21] = 1
    m[20:41, 100:301] = 1
    return m


def corner_diagonals(h, w):
    """Two pairs of pixels that touch only across a tile corner: a diagonal at (32, 256) and an anti-diagonal at (64, 512)."""
    m = np.zeros((h, w), np.uint8)
    m[31, 255] = m[32, 256] = 1
    m[63, 512] = m[64, 511] = 1
    return m


def equal_areas(h, w):
    """Three components, the two largest of six pixels each: the largest is the one with the lower root."""
    m = np.zeros((h, w), np.uint8)
    m[1:3, 1:4] = 1
    m[40:43, 300:302] = 1
    m[50, 50:55] = 1
    return m


def blobs(h, w, seed=0, n=7, speckle=2e-4):
    """A few round blobs (some overlapping, some cut by the border) and a sprinkle of single pixels; set bytes 1, 2, 128 or 255."""
    rng = np.random.default_rng([seed, h, w, 11])
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    v = np.zeros((h, w), np.float32)
    for _ in range(n):
        cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.02, 0.12) * max(h, w)
        v = np.maximum(v, np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)))
    m = (v > 0.5) | (rng.random((h, w)) < speckle)
    return np.where(m, rng.choice(BYTES, (h, w)), 0).astype(np.uint8)


def noise(h, w, seed=0, fill=0.5):
    rng = np.random.default_rng([seed, h, w, 13])
    return np.where(rng.random((h, w)) < fill, rng.choice(BYTES, (h, w)), 0).astype(np.uint8)


SEAM_MASKS = dict(spiral=spiral, comb=comb, comb_top=lambda h, w: comb(h, w, 0), u=u_shape, ring=ring_and_blob, corners=corner_diagonals,
                  ties=equal_areas, checker=checkerboard, noise=lambda h, w: noise(h, w, 1), dense=lambda h, w: noise(h, w, 2, 0.9),
                  blobs=lambda h, w: blobs(h, w, 3, speckle=2e-3), full=lambda h, w: np.full((h, w), 255, np.uint8),
                  empty=lambda h, w: np.zeros((h, w), np.uint8))


# ---- the reference: union-find over row runs, in numpy -----------------------------------------------------------------------------------
def label(mask, connectivity=8):
    """``(labels int32 [h, w] -- rank, -1 on background --, roots int64 [k], areas int64 [k], boxes int64 [k, 4] x0 y0 x1 y1)``: the
    runs of set pixels of every row, joined with the runs of the row above that they touch (8: also by a corner) by union-find with
    pointer jumping on the run numbers -- runs are numbered in row-major order, so a component's lowest run starts at its root."""
    assert connectivity in (4, 8)
    m = np.asarray(mask) != 0
    h, w = m.shape
    pad = np.zeros((h, w + 2), np.int8)
    pad[:, 1:-1] = m
    d = np.diff(pad, axis=1)                                                   # [h, w + 1]: +1 where a run starts, -1 one past its end
    ys, starts = np.nonzero(d == 1)
    ends = np.nonzero(d == -1)[1]
    n = len(ys)
    if not n:
        return np.full((h, w), -1, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 4), np.int64)
    e, stride = (1 if connectivity == 8 else 0), w + 3
    first = np.searchsorted(ys * stride + ends, (ys - 1) * stride + starts - e, side='right')      # runs of the row above that end past my start
    last = np.searchsorted(ys * stride + starts, (ys - 1) * stride + ends + e, side='left')        # ... and start before my end
    reps = np.maximum(last - first, 0)
    mine = np.repeat(np.arange(n), reps)
    theirs = np.repeat(first, reps) + (np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps))
    lab = np.arange(n)
    while True:
        a, b = lab[mine], lab[theirs]
        if (a == b).all():
            break
        np.minimum.at(lab, np.maximum(a, b), np.minimum(a, b))
        while True:
            up = lab[lab]
            if (up == lab).all():
                break
            lab = up
    heads, rank = np.unique(lab, return_inverse=True)
    k = len(heads)
    areas = np.bincount(rank, weights=ends - starts, minlength=k).astype(np.int64)
    boxes = np.empty((k, 4), np.int64)
    boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3] = w, h, -1, -1
    np.minimum.at(boxes[:, 0], rank, starts)
    np.minimum.at(boxes[:, 1], rank, ys)
    np.maximum.at(boxes[:, 2], rank, ends - 1)
    np.maximum.at(boxes[:, 3], rank, ys)
    run_of = np.cumsum((d == 1).ravel()).reshape(h, w + 1)[:, :w] - 1          # the latest run that started at or before the pixel
    labels = np.where(m, rank[np.maximum(run_of, 0)], -1).astype(np.int32)
    return labels, (ys[heads] * w + starts[heads]).astype(np.int64), areas, boxes


def label_bfs(mask, connectivity=8):
    """The same four arrays by breadth-first search from every unlabelled set pixel in row-major order (small masks only)."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    labels = np.full((h, w), -1, np.int32)
    roots, areas, boxes = [], [], []
    for y0, x0 in zip(*np.nonzero(m)):
        if labels[y0, x0] >= 0:
            continue
        k = len(roots)
        labels[y0, x0] = k
        queue, area, box = deque([(y0, x0)]), 0, [x0, y0, x0, y0]
        while queue:
            y, x = queue.popleft()
            area += 1
            box = [min(box[0], x), min(box[1], y), max(box[2], x), max(box[3], y)]
            for dy, dx in steps:
                qy, qx = y + dy, x + dx
                if 0 <= qy < h and 0 <= qx < w and m[qy, qx] and labels[qy, qx] < 0:
                    labels[qy, qx] = k
                    queue.append((qy, qx))
        roots.append(y0 * w + x0)
        areas.append(area)
        boxes.append(box)
    return labels, np.array(roots, np.int64), np.array(areas, np.int64), np.array(boxes, np.int64).reshape(-1, 4)


def sentinel(h, w):
    return [-1, 0, w, h, -1, -1]


def reference(masks, connectivity=8, min_area=0, keep=0, max_comp=256, labeller=label):
    """What ``daam_mask_components`` returns for ``masks`` [n, h, w]: ``dict(labels int32 [n, h, w], counts int32 [n, 2], comps
    int32 [n, max_comp, 6], largest int32 [n, 6], kept uint8 [n, h, w] or None)``."""
    masks = np.asarray(masks)
    n, h, w = masks.shape
    out = dict(labels=np.empty((n, h, w), np.int32), counts=np.zeros((n, 2), np.int32),
               comps=np.tile(np.array(sentinel(h, w), np.int32), (n, max_comp, 1)), largest=np.tile(np.array(sentinel(h, w), np.int32), (n, 1)),
               kept=np.zeros((n, h, w), np.uint8) if keep else None)
    for i, mask in enumerate(masks):
        labels, roots, areas, boxes = labeller(mask, connectivity)
        rows = np.concatenate([roots[:, None], areas[:, None], boxes], 1).astype(np.int32).reshape(-1, 6)
        out['labels'][i] = labels
        out['counts'][i] = (len(roots), int((areas >= min_area).sum()))
        out['comps'][i, :min(len(rows), max_comp)] = rows[:max_comp]
        if len(rows):
            big = int(areas.argmax())                                          # the first of equals: the lowest root
            out['largest'][i] = rows[big]
            if keep == 1:
                out['kept'][i] = (labels >= 0) & (areas[np.maximum(labels, 0)] >= min_area)
            elif keep == 2:
                out['kept'][i] = labels == big
    return out


# ---- the kernels' union rules, pixel by pixel --------------------------------------------------------------------------------------------
def rule_unions(mask, connectivity=8, tile=TILE):
    """The set of unions ``neighbour_unions`` (daam_components.hip) makes: the local kernel's (both pixels in one tile, pixels
    outside the tile seen as clear, `left` only at a 32-column word's first pixel: inside a word the run start stands for it) and the
    seam kernel's (true neighbours, pixels in different tiles; top row, left column, right column of a tile).  Returns ``(local,
    seam)`` lists of ``((y, x), (qy, qx))``; their closure with the word runs must be the reference's components."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    conn8 = connectivity == 8
    tile_of = lambda y, x: (y // tile[0], x // tile[1])

    def unions(y, x, is_set, with_left):
        got = []
        l, u = is_set(y, x - 1), is_set(y - 1, x)
        if l and with_left:
            got.append((y, x - 1))
        if u:
            if not (l and is_set(y - 1, x - 1)):
                got.append((y - 1, x))
        elif conn8:
            if not l and is_set(y - 1, x - 1):
                got.append((y - 1, x - 1))
            if not is_set(y, x + 1) and is_set(y - 1, x + 1):
                got.append((y - 1, x + 1))
        return got
    everywhere = lambda y, x: 0 <= y < h and 0 <= x < w and bool(m[y, x])
    local, seam = [], []
    for y, x in zip(*np.nonzero(m)):
        inside = lambda qy, qx: everywhere(qy, qx) and tile_of(qy, qx) == tile_of(y, x)
        local += [((y, x), q) for q in unions(y, x, inside, x % 32 == 0)]
        on_edge = (y % tile[0] == 0 and y > 0) or (x % tile[1] == 0 and x > 0) or (x % tile[1] == tile[1] - 1 and x + 1 < w)
        if on_edge:
            seam += [((y, x), q) for q in unions(y, x, everywhere, True) if tile_of(*q) != tile_of(y, x)]
    return local, seam


def closure_labels(mask, unions):
    """int32 [h, w]: rank labels of the closure of ``unions`` and the runs inside 32-column words (what the local kernel starts from)."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    parent = np.arange(h * w)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    pairs = [(y * w + x, qy * w + qx) for (y, x), (qy, qx) in unions]
    pairs += [(y * w + x, y * w + x - 1) for y, x in zip(*np.nonzero(m)) if x % 32 and m[y, x - 1]]
    for a, b in pairs:
        a, b = find(a), find(b)
        parent[max(a, b)] = min(a, b)
    roots = np.array([find(i) for i in range(h * w)]).reshape(h, w)
    uniq = np.unique(roots[m])
    return np.where(m, np.searchsorted(uniq, roots), -1).astype(np.int32)


# ---- a numpy stand-in of libdaam_components -------------------------------------------------------------------------------------------------
class FakeComponentsLib:
    """``daam_mask_components`` / ``_workspace`` in numpy on CPU tensors' memory, held to the header's limits; records every call's
    ``(n_masks, connectivity, min_area, keep, max_comp, labels asked for)``."""

    def __init__(self):
        self.calls = []

    def daam_mask_components_workspace(self, n_masks, h, w, max_comp):
        ok = 0 <= n_masks <= 32 and h >= 1 and w >= 1 and h * w < 2 ** 31 and 0 <= max_comp <= 65536
        r8 = lambda b: (b + 7) // 8 * 8
        return 512 + 2 * r8(4 * n_masks * h * w) + r8(4 * n_masks * h * -(-w // 256)) if ok else 0

    def daam_mask_components(self, masks, n_masks, h, w, connectivity, min_area, keep, max_comp, labels, counts, comps, largest, kept,
                             ws, ws_bytes, stream):
        assert ws_bytes >= self.daam_mask_components_workspace(n_masks, h, w, max_comp) > 0 and ws and ws % 8 == 0
        assert connectivity in (4, 8) and min_area >= 0 and keep in (0, 1, 2) and 1 <= n_masks
        assert masks and counts and largest and (comps is None) == (max_comp == 0) and (kept is None) == (keep == 0)
        self.calls.append((n_masks, connectivity, min_area, keep, max_comp, labels is not None))
        stack = S._array(masks, ctypes.c_uint8, n_masks * h * w).reshape(n_masks, h, w)
        want = reference(stack, connectivity, min_area, keep, max_comp)
        if labels is not None:
            S._array(labels, ctypes.c_int32, n_masks * h * w)[:] = want['labels'].ravel()
        S._array(counts, ctypes.c_int32, n_masks * 2)[:] = want['counts'].ravel()
        if max_comp:
            S._array(comps, ctypes.c_int32, n_masks * max_comp * 6)[:] = want['comps'].ravel()
        S._array(largest, ctypes.c_int32, n_masks * 6)[:] = want['largest'].ravel()
        if keep:
            S._array(kept, ctypes.c_uint8, n_masks * h * w)[:] = want['kept'].ravel()
        return 0


def fake_word_masks(calls):
    """``engine.word_masks`` in numpy (``_epilogue_domain.emulate_expand``): masks alone; every call's threshold goes to ``calls``."""
    import torch

    def word_masks(maps, idx_lists, out_h, out_w, absolute=False, threshold=0.4, labels=True):
        calls.append(float(threshold))
        planes = torch.stack([maps[list(i)].mean(0) for i in idx_lists]).contiguous()
        masks = np.stack([D.emulate_expand(p, out_h, out_w, absolute=absolute) > np.float32(threshold) for p in planes.numpy()])
        return planes, torch.from_numpy(masks.astype(np.uint8)), None
    return word_masks


def install(setattr_):
    """``_locate_domain.install`` (CPU tensors pass for device tensors, a ``FakeLocateLib``) plus a ``FakeComponentsLib`` under
    ``daam_amd.engine`` and a numpy ``engine.word_masks``.  Returns ``(engine module, components lib, locate lib, the thresholds of
    the word_masks calls)``."""
    E, locate = L.install(setattr_)
    lib = FakeComponentsLib()
    setattr_(E.nat, 'load_components', lambda: lib)
    thresholds = []
    setattr_(E, 'word_masks', fake_word_masks(thresholds))
    return E, lib, locate, thresholds
