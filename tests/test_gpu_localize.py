"""``daam_localize`` (include/daam_locate.h) on the device, through ctypes and through ``GlobalHeatMap``.

The call restates the arithmetic of ``daam_word_masks``, so against that route -- the numpy box of the masks
``daam_word_masks(threshold=t)`` writes, once per threshold -- every box is held to integer equality, the peak to the first arg-max of
``expand_word_map(absolute=True)`` and the three peak values to its bits.  The test that does not lean on the sibling kernels is
``test_boxes_against_the_float64_oracle``: every box contains the box of the pixels ``_epilogue_domain.expand`` puts surely above the
threshold and lies inside the box of those plus the ambiguous ones (``test_localize_cpu.py`` caps how many those are)."""
import ctypes

import numpy as np
import pytest
import torch

import _epilogue_domain as D
import _locate_domain as L
import _sweep_domain as S
from oracle import fake_diffusers as fd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64                       # guard bytes on either side of a buffer
# (words, truth masks, thresholds): every W of {0, 1, 3, 32}, G of {0, 1, 5, 32}, T of {0, 1, 21, 64}
COMBOS = [(0, 1, 0), (1, 0, 1), (3, 1, 21), (32, 5, 64), (3, 32, 0), (1, 5, 64), (32, 0, 1), (0, 5, 21)]


def _guarded(n_bytes, fill, offset=0):
    """A uint8 device buffer of ``n_bytes`` at ``offset`` bytes past 16-byte alignment, between two guards of 0xA5, filled with ``fill``."""
    raw = torch.full((GUARD + 16 + n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(raw.data_ptr() + GUARD) % 16) + offset
    raw[start:start + n_bytes] = fill
    return raw, start


def _guards_intact(raw, start, n_bytes):
    return bool((raw[:start] == 0xA5).all()) and bool((raw[start + n_bytes:] == 0xA5).all())


def localize_raw(planes, out, thr, truth=None, absolute=False, truth_offset=0, ws_offset=0):
    """One ``daam_localize`` call through ctypes on guarded buffers: outputs pre-filled with 0xFF, a workspace of exactly the bytes
    asked for, the truth stack at ``truth_offset`` bytes past alignment.  Returns numpy ``(boxes, peaks, peak_values, truth_boxes,
    hits)`` (None where the call has none) after checking every guard."""
    from daam_amd import _native as nat
    lib = nat.load_locate()
    n = 0 if planes is None else len(planes)
    if n:
        planes = torch.as_tensor(np.ascontiguousarray(planes), dtype=torch.float32).to(DEV).contiguous()
    h, w = planes.shape[1:] if n else (1, 1)
    g, t = (0 if truth is None else len(truth)), len(thr)
    oh, ow = out
    need = lib.daam_localize_workspace(n, g, t, oh, ow)
    assert need > 0 and need % 8 == 0
    sizes = dict(ws=need, boxes=16 * n * t, peaks=8 * n, values=12 * n, tboxes=16 * g, hits=n * g, truth=g * oh * ow)
    bufs = {k: _guarded(v, 0x5A if k == 'ws' else 0xFF, ws_offset if k == 'ws' else 0) for k, v in sizes.items() if v and k != 'truth'}
    if g:
        bufs['truth'] = raw, start = _guarded(g * oh * ow, 0, truth_offset)
        raw[start:start + g * oh * ow] = torch.as_tensor(np.ascontiguousarray(truth), dtype=torch.uint8).to(DEV).reshape(-1)
        before = raw.clone()
    ptr = lambda k: bufs[k][0].data_ptr() + bufs[k][1] if k in bufs else None
    nat.check_locate(lib.daam_localize(planes.data_ptr() if n else None, n, h, w, oh, ow, 1 if absolute else 0,
                                       (ctypes.c_float * max(t, 1))(*thr), t, ptr('truth'), g, ptr('boxes'), ptr('peaks'), ptr('values'),
                                       ptr('tboxes'), ptr('hits'), ptr('ws'), need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for k, (raw, start) in bufs.items():
        assert _guards_intact(raw, start, sizes[k]), f'guard bytes around {k} changed'
    if g:
        assert torch.equal(bufs['truth'][0], before), 'the truth bytes changed'

    def arr(k, dtype, shape):
        if k not in bufs:
            return None
        raw, start = bufs[k]
        return raw[start:start + sizes[k]].cpu().numpy().view(dtype).reshape(shape)
    return (arr('boxes', np.int32, (n, t, 4)), arr('peaks', np.int32, (n, 2)), arr('values', np.float32, (n, 3)),
            arr('tboxes', np.int32, (g, 4)), arr('hits', np.uint8, (n, g)))


def route(planes, out, thr, absolute=False):
    """The existing route: per threshold the numpy boxes of the masks ``daam_word_masks`` writes; per word the first arg-max,
    the value, the minimum and the maximum of ``expand_word_map(absolute=True)`` on the host copy."""
    from daam_amd import engine as E
    planes = torch.as_tensor(np.ascontiguousarray(planes), dtype=torch.float32).to(DEV).contiguous()
    n = planes.shape[0]
    boxes = np.zeros((n, len(thr), 4), np.int32)
    for t, tau in enumerate(thr):
        _, masks, _ = E.word_masks(planes, [[j] for j in range(n)], out[0], out[1], absolute=absolute, threshold=float(tau), labels=False)
        boxes[:, t] = L.mask_boxes(masks.cpu().numpy())
    peaks, values = np.zeros((n, 2), np.int32), np.zeros((n, 3), np.float32)
    for j in range(n):
        v = E.expand_word_map(planes[j], out[0], out[1], absolute=True).cpu().numpy()
        at = int(v.argmax())
        peaks[j] = (at % out[1], at // out[1])
        values[j] = (v.reshape(-1)[at],) + tuple(L.lo_hi(v))
    return boxes, peaks, values


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _assert_route(got, planes, out, thr, truth, absolute, what):
    boxes, peaks, values, truth_boxes, hits = got
    if planes is not None and len(planes):
        want = route(planes, out, thr, absolute)
        if len(thr):
            assert np.array_equal(boxes, want[0]), f'{what}: boxes differ at {int((boxes != want[0]).any(-1).sum())} of {boxes.shape[0] * boxes.shape[1]}'
        else:
            assert boxes is None
        assert np.array_equal(peaks, want[1]), (what, peaks, want[1])
        assert np.array_equal(_bits(values), _bits(want[2])), (what, values, want[2])
    else:
        assert boxes is None and peaks is None and values is None
    if truth is not None:
        assert np.array_equal(truth_boxes, L.mask_boxes(truth)), what
        if peaks is not None:
            assert np.array_equal(hits, np.array([[truth[g, y, x] != 0 for g in range(len(truth))] for x, y in peaks], np.uint8)), what
        else:
            assert hits is None
    else:
        assert truth_boxes is None and hits is None


# ---- exact against the existing route ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('combo', COMBOS, ids=lambda c: 'W%d-G%d-T%d' % c)
@pytest.mark.parametrize('absolute', [False, True], ids=['minmax', 'absolute'])
@pytest.mark.parametrize('sizes', S.SIZES, ids=lambda s: '%dx%d-%dx%d' % (s[0] + s[1]))
def test_results_equal_the_existing_route(sizes, absolute, combo):
    n_words, n_truth, n_thr = combo
    planes = S.word_planes(n_words, *sizes[0], seed=n_thr) if n_words else None
    truth = S.truth_stack(n_truth, *sizes[1], seed=n_words) if n_truth else None
    thr = S.thresholds(n_thr) if n_thr else []
    got = localize_raw(planes, sizes[1], thr, truth, absolute)
    _assert_route(got, planes, sizes[1], thr, truth, absolute, (sizes, absolute, combo))


def test_the_full_call_equals_the_existing_route():
    """32 words x 32 truth masks x 64 thresholds, given in descending order."""
    sizes = S.FULL_SIZE
    planes, truth, thr = S.word_planes(32, *sizes[0], seed=9), S.truth_stack(32, *sizes[1], seed=9), S.thresholds(64)[::-1]
    for absolute in (False, True):
        _assert_route(localize_raw(planes, sizes[1], thr, truth, absolute), planes, sizes[1], thr, truth, absolute, ('full', absolute))


def test_many_tiles_in_both_directions():
    """64 x 64 -> 512 x 768: three tile columns of 256, and tile rows whatever the row count of a tile."""
    sizes = L.BIG_SIZE
    planes, truth, thr = S.word_planes(3, *sizes[0], seed=11), S.truth_stack(2, *sizes[1], seed=11), S.thresholds(21)
    for absolute in (False, True):
        _assert_route(localize_raw(planes, sizes[1], thr, truth, absolute), planes, sizes[1], thr, truth, absolute, ('big', absolute))


# ---- the planes of _locate_domain ----------------------------------------------------------------------------------------------------------
def test_two_equal_peaks_constant_plane_and_edge_truth():
    plane, first, second = L.two_peaks()
    h, w = plane.shape
    thr = [0.5, 1.5, -0.25]
    truth = L.edge_truth(h, w)
    boxes, peaks, values, truth_boxes, hits = got = localize_raw(plane[None], (h, w), thr, truth)        # identity size
    _assert_route(got, plane[None], (h, w), thr, truth, False, 'two peaks')
    assert tuple(peaks[0]) == (first[1], first[0]) and values[0].tolist() == [2.0, 0.0, 2.0]
    assert boxes[0].tolist() == [[second[1], first[0], first[1], second[0]], [w, h, -1, -1], [0, 0, w - 1, h - 1]]     # 1.5: empty; -0.25: all
    assert truth_boxes.tolist() == [[w, h, -1, -1], [w - 1, h - 1, w - 1, h - 1]] and not hits.any()
    # a peak in the last row and column hits the one-pixel mask
    corner = np.zeros((h, w), np.float32)
    corner[-1, -1] = 1
    got = localize_raw(corner[None], (h, w), [0.5], truth)
    assert tuple(got[1][0]) == (w - 1, h - 1) and got[4].tolist() == [[0, 1]] and got[0][0, 0].tolist() == [w - 1, h - 1, w - 1, h - 1]
    # a constant plane at its own size and a plane of zeros resized: min-max makes every pixel exactly 0; the peak is pixel 0
    for planes, out in ((L.constant_plane()[None], (5, 7)), (np.zeros((2, 5, 7), np.float32), (9, 11))):
        boxes, peaks, values, _, _ = got = localize_raw(planes, out, [-0.25, 0.0, 0.4])
        _assert_route(got, planes, out, [-0.25, 0.0, 0.4], None, False, 'constant')
        assert (boxes == [[0, 0, out[1] - 1, out[0] - 1], [out[1], out[0], -1, -1], [out[1], out[0], -1, -1]]).all() and not peaks.any()
        assert (values == planes.reshape(len(planes), -1)[:, :1]).all()


def test_a_single_output_pixel():
    planes = S.word_planes(2, 8, 8, seed=3)
    truth = np.array([[[7]], [[0]]], np.uint8)
    boxes, peaks, values, truth_boxes, hits = got = localize_raw(planes, (1, 1), [-0.25, 0.0], truth)
    _assert_route(got, planes, (1, 1), [-0.25, 0.0], truth, False, '1 x 1')
    assert (boxes == [[0, 0, 0, 0], [1, 1, -1, -1]]).all() and not peaks.any() and (values[:, 0] == values[:, 1]).all()
    assert truth_boxes.tolist() == [[0, 0, 0, 0], [1, 1, -1, -1]] and hits.tolist() == [[1, 0], [1, 0]]


# ---- the float64 oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(S.oracle_cases()), ids=lambda c: '%dx%d-%dx%d-%s-%s' % (c[0][0] + c[0][1] + (c[1][0], 'abs' if c[2] else 'minmax')))
def test_boxes_against_the_float64_oracle(case):
    sizes, kinds, absolute, thr = case
    planes = S.oracle_planes(sizes, kinds)
    boxes, peaks, values, _, _ = localize_raw(planes, sizes[1], list(thr), None, absolute)
    for j, plane in enumerate(planes):
        o = L.oracle_boxes(plane, *sizes[1], absolute, thr)
        assert not o['ill']
        print(f'{sizes} {kinds[j]} absolute={absolute}: boxes {boxes[j].tolist()} inner {o["inner"].tolist()} outer {o["outer"].tolist()}')
        for t in range(len(thr)):
            assert L.contains(boxes[j, t], o['inner'][t]) and L.contains(o['outer'][t], boxes[j, t]), (kinds[j], thr[t], boxes[j, t], o['inner'][t], o['outer'][t])
        ref = D.expand(plane, *sizes[1], absolute=True)
        val, bound = ref['value'], ref['value_bound']
        top = np.unravel_index(int(val.argmax()), val.shape)
        x, y = peaks[j]
        assert val[top] - val[y, x] <= bound[y, x] + bound[top], (kinds[j], (x, y), top)
        assert abs(float(values[j, 0]) - val[y, x]) <= bound[y, x] and abs(float(values[j, 1]) - val.min()) <= bound.max()


# ---- truth bytes, workspace ---------------------------------------------------------------------------------------------------------------
def test_truth_bytes_at_any_alignment():
    """A stack at odd byte offsets with an odd plane size (37 x 53 = 1961) and a wide one (333 = 20 chunks and two edges); the set
    bytes are 1, 2, 128 and 255; a workspace 8 bytes past 16-byte alignment."""
    for sizes in (S.FULL_SIZE, ((64, 64), (200, 333))):
        planes, thr = S.word_planes(3, *sizes[0], seed=2), S.thresholds(21)
        truth = np.concatenate([S.truth_stack(5, *sizes[1], seed=4), L.edge_truth(*sizes[1])])
        assert {1, 2, 128, 255} <= set(np.unique(truth))
        ones = (truth != 0).astype(np.uint8)
        base = localize_raw(planes, sizes[1], thr, ones)
        assert np.array_equal(base[3], L.mask_boxes(truth))
        for offset in (1, 3, 7, 15):
            got = localize_raw(planes, sizes[1], thr, truth, truth_offset=offset)
            assert all(np.array_equal(a, b) for a, b in zip(got, base)), offset
            only = localize_raw(None, sizes[1], [], truth, truth_offset=offset)
            assert np.array_equal(only[3], base[3]) and only[0] is None and only[4] is None
        got = localize_raw(planes, sizes[1], thr, truth, ws_offset=8)
        assert all(np.array_equal(a, b) for a, b in zip(got, base))


# ---- independence -----------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_rest_of_the_call():
    sizes = ((64, 64), (200, 333))
    planes, truth, thr = S.word_planes(32, *sizes[0], seed=1), S.truth_stack(5, *sizes[1], seed=1), S.thresholds(21)
    full = localize_raw(planes, sizes[1], thr, truth)
    again = localize_raw(planes, sizes[1], thr, truth)
    assert all(np.array_equal(a, b) for a, b in zip(again, full)), 'a second run'
    for j in (0, 13, 31):                                          # a word alone
        alone = localize_raw(planes[j:j + 1], sizes[1], thr, truth)
        assert all(np.array_equal(alone[k][0], full[k][j]) for k in (0, 1, 2, 4)) and np.array_equal(alone[3], full[3])
    pick = [20, 3, 8, 3, 0]                                        # a permuted subset with a duplicate: the same boxes
    sub = localize_raw(planes, sizes[1], [thr[i] for i in pick], truth)
    assert np.array_equal(sub[0], full[0][:, pick]) and all(np.array_equal(sub[k], full[k]) for k in (1, 2, 3, 4))
    none = localize_raw(planes, sizes[1], thr, None)                # no truth masks
    assert none[3] is None and none[4] is None and all(np.array_equal(none[k], full[k]) for k in (0, 1, 2))
    one = localize_raw(planes, sizes[1], thr, truth[2:3])           # a truth mask alone
    assert np.array_equal(one[3][0], full[3][2]) and np.array_equal(one[4][:, 0], full[4][:, 2]) and np.array_equal(one[0], full[0])


# ---- Python -------------------------------------------------------------------------------------------------------------------------------
class _Image:
    def __init__(self, width, height):
        self.size = (width, height)             # PIL order


PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


def _ghm(h, w):
    from daam_amd import GlobalHeatMap
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:h, 0:w]
    maps = np.stack([np.exp(-((yy - rng.uniform(0, h)) ** 2 + (xx - rng.uniform(0, w)) ** 2) / (2 * (0.2 * h) ** 2)) +
                     0.05 * np.abs(rng.standard_normal((h, w))) for _ in range(13)]).astype(np.float32)
    return GlobalHeatMap(fd.FakeTokenizer(), PROMPT, torch.from_numpy(maps).to(DEV))


def test_global_heat_map_localize_equals_segment():
    from daam_amd import LocalizationEvaluator, mask_boxes
    ghm = _ghm(16, 24)
    words, image = ['monkey', 'bicycle', ('photo', None)], _Image(53, 37)
    truth_np = S.truth_stack(4, 37, 53, seed=8)
    truth = torch.from_numpy(truth_np).to(DEV)
    thr = [0.1, 0.4, 0.75, 1.5]
    loc = ghm.localize(words, image, thr, truth)
    assert loc.boxes.is_cuda and loc.boxes.dtype == torch.int32 and loc.boxes.shape == (3, 4, 4) and loc.hits.dtype == torch.bool
    assert loc.size == (37, 53) and loc.peaks.shape == (3, 2) and loc.peak_values.shape == (3, 3)
    for t, tau in enumerate(thr):
        seg = ghm.segment(words, image, threshold=tau, labels=False)
        want = L.mask_boxes(seg.masks.cpu().numpy())
        assert np.array_equal(loc.boxes[:, t].cpu().numpy(), want)
        assert np.array_equal(mask_boxes(seg.masks).cpu().numpy(), want)
        for w, word in enumerate(words[:2]):
            assert loc.box(word, tau) == (None if want[w, 2] < 0 else tuple(int(v) for v in want[w]))
    assert np.array_equal(loc.truth_boxes.cpu().numpy(), L.mask_boxes(truth_np)) and torch.equal(mask_boxes(truth), loc.truth_boxes)
    host = loc.cpu()
    boxes, peaks, tb = host.boxes.numpy(), host.peaks.numpy(), host.truth_boxes.numpy()
    for w, word in enumerate(words):
        heat = ghm.compute_word_heat_map(*((word, None) if isinstance(word, str) else word))
        v = heat.expand_as(image, absolute=True).numpy()
        assert int(peaks[w, 1]) * 53 + int(peaks[w, 0]) == int(v.argmax()) and float(host.peak_values[w, 0]) == float(v.max())
    assert np.array_equal(loc.pointing().cpu().numpy(), np.array([[truth_np[g, y, x] != 0 for g in range(4)] for x, y in peaks]))
    brute = np.array([[[L.box_iou(boxes[w, t], tb[g]) for t in range(4)] for g in range(4)] for w in range(3)], np.float32)
    assert np.array_equal(loc.box_iou().cpu().numpy(), brute) and (brute[:, :, 3] == 0).all()
    ev = LocalizationEvaluator().log(loc)
    assert len(ev) == 3 and np.array_equal(ev.corloc, (brute.max(1) >= 0.5).mean(0).astype(np.float32))
    as_seg = ghm.localize(words, image, truth=ghm.segment(['riding', 'a'], image, labels=False), absolute=True)
    assert as_seg.boxes.shape == (3, 1, 4) and as_seg.hits.shape == (3, 2)
