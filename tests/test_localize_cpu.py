"""Localisation (``daam_localize``, include/daam_locate.h) without a GPU: ``libdaam_locate.so`` builds beside the other
libraries and exports what its header declares and the binding names; the header is C99; no kernel has scratch; every argument the
header rules out is refused before any HIP call; the lemma the design rests on -- a row holds a mask pixel iff its normalised maximum
exceeds the threshold -- in f32 numpy over every case; the numpy restatement against brute force; the Python layer
(``engine.localize``, ``evaluate.mask_boxes``, ``GlobalHeatMap.localize``, ``Localization``, ``LocalizationEvaluator``) on a numpy
stand-in of the library; and, on the float64 oracle alone, that the cases ``test_gpu_localize.py`` holds to it leave few pixels
ambiguous.  The kernels run in that file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _epilogue_domain as D
import _libcheck as LC
import _locate_domain as L
import _sweep_domain as S
from oracle import fake_diffusers as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('locate_init_kernel', 'locate_profile_kernel', 'locate_truth_kernel', 'locate_boxes_kernel')
E_INVALID = -1


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build(verbose=False)
    return build.LOCATE_LIB


@pytest.fixture(scope='module')
def lib(built):
    from daam_amd import _native as nat
    return nat.load_locate()


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_library_builds_and_exports_its_header(built, lib):
    from daam_amd import _native as nat, build
    assert os.path.exists(built) and os.path.basename(built) == 'libdaam_locate.so' and not build.locate_stale()
    assert build.LOCATE_SOURCES == ['daam_locate.hip']
    exported = LC.exported(built)
    assert exported == LC.declared('daam_locate.h') == sorted(nat.LOCATE_EXPORTS) and len(exported) == 4
    assert lib.daam_locate_abi_version() == 1 == nat.LOCATE_ABI_VERSION
    assert len(lib.daam_localize.argtypes) == 19
    assert nat.LOCATE_LIB_PATH == built or os.environ.get('DAAM_LOCATE_LIB')
    names = list(build.kernel_shas(built))
    assert sorted(sum(k in n for n in names) for k in KERNELS) == [1, 1, 1, 1] and len(names) == 4


def test_locate_header_is_c99(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "daam_locate.h"\nint main(void) { return DAAM_LOCATE_ABI_VERSION == 1 && sizeof(&daam_localize) ? 0 : 1; }\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o',
                    str(tmp_path / 'use.o')], check=True)


def test_no_kernel_has_scratch(built):
    """Private segment size 0 and the private-segment enable bit clear in every kernel descriptor."""
    from daam_amd import build
    names = list(build.kernel_shas(built))
    assert len(names) == 4
    LC.assert_no_scratch(built, names)


# ---- argument checks: all of them before any HIP call, so they run here ---------------------------------------------------------------
def _call(lib, **over):
    """A call that is in range but for ``over``; pointers are small fake addresses (nothing is dereferenced but ``thresholds``)."""
    a = dict(word_maps=0x1000, n_words=3, h=16, w=24, out_h=37, out_w=53, absolute=0, thresholds=[0.9, 0.1, 0.1], truth=0x2000,
             n_truth=2, boxes=0x3000, peaks=0x4000, peak_values=0x5000, truth_boxes=0x7000, hits=0x8000, workspace=0x6000,
             workspace_bytes=None, stream=None)
    a.update(over)
    thr = a['thresholds']
    arr = None if thr is None else (ctypes.c_float * max(len(thr), 1))(*thr)
    n_thr = a.get('n_thr', 0 if thr is None else len(thr))
    if a['workspace_bytes'] is None:
        a['workspace_bytes'] = lib.daam_localize_workspace(a['n_words'], a['n_truth'], n_thr, a['out_h'], a['out_w']) or 1 << 20
    rc = lib.daam_localize(a['word_maps'], a['n_words'], a['h'], a['w'], a['out_h'], a['out_w'], a['absolute'], arr, n_thr, a['truth'],
                           a['n_truth'], a['boxes'], a['peaks'], a['peak_values'], a['truth_boxes'], a['hits'], a['workspace'],
                           a['workspace_bytes'], a['stream'])
    return rc, lib.daam_locate_last_error().decode()


NO_WORDS = dict(n_words=0, word_maps=None, peaks=None, peak_values=None, boxes=None, hits=None)
BAD = {
    'NULL word_maps': dict(word_maps=None), 'NULL thresholds': dict(thresholds=None, n_thr=3), 'NULL boxes': dict(boxes=None),
    'NULL peaks': dict(peaks=None), 'NULL peak_values': dict(peak_values=None), 'NULL workspace': dict(workspace=None),
    'NULL truth with masks': dict(truth=None), 'NULL truth_boxes with masks': dict(truth_boxes=None), 'NULL hits with masks': dict(hits=None),
    'truth without masks': dict(n_truth=0, hits=None, truth_boxes=None), 'hits without masks': dict(n_truth=0, truth=None, truth_boxes=None),
    'truth_boxes without masks': dict(n_truth=0, truth=None, hits=None), 'boxes without thresholds': dict(thresholds=[], n_thr=0),
    'word_maps without words': dict(NO_WORDS, word_maps=0x1000), 'peaks without words': dict(NO_WORDS, peaks=0x4000),
    'boxes without words': dict(NO_WORDS, boxes=0x3000), 'hits without words': dict(NO_WORDS, hits=0x8000),
    'nothing to do': dict(NO_WORDS, n_truth=0, truth=None, truth_boxes=None), '-1 words': dict(n_words=-1), '33 words': dict(n_words=33),
    '33 truth masks': dict(n_truth=33), '-1 truth masks': dict(n_truth=-1), 'h 0': dict(h=0), 'w 129': dict(w=129), 'h 129': dict(h=129),
    'out_h 0': dict(out_h=0), 'out_w 0': dict(out_w=0), '2^31 pixels': dict(out_h=1 << 16, out_w=1 << 15),
    '-1 thresholds': dict(n_thr=-1), '65 thresholds': dict(thresholds=[i / 65 for i in range(65)]),
    'nan': dict(thresholds=[0.1, float('nan'), 0.9]), 'inf': dict(thresholds=[0.1, 0.4, float('inf')]),
    '-inf': dict(thresholds=[float('-inf'), 0.4, 0.9]), 'small workspace': dict(workspace_bytes=512 + 4 * 3 * 90 - 1),
    'unaligned workspace': dict(workspace=0x6004),
}


@pytest.mark.parametrize('what', sorted(BAD))
def test_out_of_range_is_refused_before_any_hip_call(lib, what):
    rc, msg = _call(lib, **BAD[what])
    assert rc == E_INVALID and msg, (what, rc, msg)


def test_workspace_is_monotone_and_zero_out_of_range(lib):
    ws = lib.daam_localize_workspace
    assert ws(3, 2, 3, 37, 53) == 512 + 4 * 3 * 90 == L.FakeLocateLib().daam_localize_workspace(3, 2, 3, 37, 53)
    assert ws(0, 1, 0, 37, 53) == 512 and ws(1, 0, 0, 1, 2) == 512 + 16 and ws(1, 0, 0, 1, 2) % 8 == 0
    for bad in ((0, 0, 1, 4, 4), (33, 1, 1, 4, 4), (-1, 1, 1, 4, 4), (1, -1, 1, 4, 4), (1, 33, 1, 4, 4), (1, 1, -1, 4, 4), (1, 1, 65, 4, 4),
                (1, 1, 1, 0, 4), (1, 1, 1, 4, 0), (1, 1, 1, 1 << 16, 1 << 15)):
        assert ws(*bad) == 0, bad
    assert ws(32, 32, 64, 46340, 46340) == 512 + 4 * 32 * 2 * 46340
    assert ws(32, 0, 0, (1 << 31) - 1, 1) == 512 + 4 * 32 * (1 << 31)
    grid = [(1, 2, 31, 32), (0, 1, 31, 32), (0, 1, 63, 64), (1, 37, 4096), (1, 53, 4096)]
    base = [g[0] for g in grid]
    for axis, values in enumerate(grid):
        sizes = [ws(*(base[:axis] + [v] + base[axis + 1:])) for v in values]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (axis, sizes)


# ---- the lemma, and the restatement against brute force ----------------------------------------------------------------------------------
ALL_THRESHOLDS = sorted(set(S.thresholds(64)) | set(S.thresholds(21)) | {float(t) for t in S.ORACLE_FULL})


@pytest.mark.parametrize('sizes', S.SIZES, ids=lambda s: '%dx%d-%dx%d' % (s[0] + s[1]))
def test_normalised_maximum_exceeds_a_threshold_iff_a_pixel_does(sizes):
    """``q(max of a row) > tau`` <=> ``any(q(v) > tau)`` on that row, and the same for columns: q is non-decreasing in f32."""
    thr = np.asarray(ALL_THRESHOLDS, np.float32)
    for j, kind in enumerate(S.WORD_KINDS):
        raw = D.emulate_resize(D.word_plane(kind, *sizes[0], seed=j), *sizes[1]).astype(np.float32)
        lo, hi = L.lo_hi(raw)
        v = L.q(raw, lo, hi)
        assert (np.diff(L.q(np.sort(raw.reshape(-1)), lo, hi)) >= 0).all(), kind            # monotone on the plane's own values
        for axis in (0, 1):
            of_max = L.q(raw.max(axis), lo, hi)[:, None] > thr[None]
            any_px = (np.moveaxis(v, axis, -1)[..., None] > thr).any(1)
            assert np.array_equal(of_max, any_px), (sizes, kind, axis)


@pytest.mark.parametrize('absolute', [False, True], ids=['minmax', 'absolute'])
@pytest.mark.parametrize('sizes', S.SIZES, ids=lambda s: '%dx%d-%dx%d' % (s[0] + s[1]))
def test_restatement_equals_brute_force(sizes, absolute):
    planes = S.word_planes(7, *sizes[0], seed=4)
    truth = S.truth_stack(3, *sizes[1], seed=2)
    raw = L.raw_of(planes, *sizes[1])
    thr = S.thresholds(21) + [1.5, -0.25]
    boxes, peaks, values, truth_boxes, hits = L.restate(raw, thr, absolute, truth)
    assert np.array_equal(boxes, L.brute_boxes(raw, thr, absolute))
    want = D.emulate_expand  # the values the masks compare, pixel by pixel
    for j, plane in enumerate(planes):
        v = want(plane, *sizes[1], absolute=absolute)
        assert all(L.box_of(v > np.float32(t)) == boxes[j, k].tolist() for k, t in enumerate(thr))
        assert raw[j, peaks[j, 1], peaks[j, 0]] == raw[j].max() == values[j, 0] == values[j, 2] and values[j, 1] == raw[j].min()
        assert int(peaks[j, 1]) * sizes[1][1] + int(peaks[j, 0]) == int(raw[j].argmax())
    for g, m in enumerate(truth):
        ys, xs = np.nonzero(m)
        assert truth_boxes[g].tolist() == [xs.min(), ys.min(), xs.max(), ys.max()]
        assert [int(h) for h in hits[:, g]] == [int(m[y, x] != 0) for x, y in peaks]


def test_restatement_on_the_extra_planes():
    plane, first, second = L.two_peaks()
    raw = plane[None]
    boxes, peaks, values, truth_boxes, hits = L.restate(raw, [0.5, 1.5, -0.25], False, L.edge_truth(*plane.shape))
    assert tuple(peaks[0]) == (first[1], first[0]) and first[0] < second[0] and first[1] > second[1]
    assert boxes[0, 0].tolist() == [second[1], first[0], first[1], second[0]]                 # both maxima, nothing else above 0.5
    assert boxes[0, 1].tolist() == [plane.shape[1], plane.shape[0], -1, -1] and boxes[0, 2].tolist() == [0, 0, plane.shape[1] - 1, plane.shape[0] - 1]
    assert truth_boxes.tolist() == [[plane.shape[1], plane.shape[0], -1, -1], [plane.shape[1] - 1, plane.shape[0] - 1] * 2] and not hits.any()
    flat = L.restate(L.constant_plane()[None], [0.0, -0.25], False)
    assert flat[0][0].tolist() == [[7, 5, -1, -1], [0, 0, 6, 4]] and tuple(flat[1][0]) == (0, 0) and flat[2][0].tolist() == [0.25] * 3
    zeros = np.array([[0.0, -0.0], [-0.0, 0.0]], np.float32)                                   # -0 sorts below +0
    _, peaks, values, _, _ = L.restate(zeros[None], [], True)
    assert tuple(peaks[0]) == (0, 0) and not np.signbit(values[0, 0]) and np.signbit(values[0, 1])


# ---- the Python layer on the numpy stand-in -------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    return L.install(monkeypatch.setattr)


def _inputs(n_words, n_truth, sizes=((6, 10), (12, 17)), seed=5):
    planes = torch.from_numpy(S.word_planes(n_words, *sizes[0], seed=seed))
    truth = torch.from_numpy(S.truth_stack(n_truth, *sizes[1], seed=seed)) if n_truth else None
    return planes, truth


def _same(got, want):
    boxes, peaks, values, truth_boxes, hits = got
    assert boxes.dtype == peaks.dtype == torch.int32 and values.dtype == torch.float32
    assert np.array_equal(boxes.numpy(), want[0]) and np.array_equal(peaks.numpy(), want[1]) and np.array_equal(values.numpy(), want[2])
    assert (truth_boxes is None) == (want[3] is None) == (hits is None)
    if hits is not None:
        assert truth_boxes.dtype == torch.int32 and hits.dtype == torch.bool
        assert np.array_equal(truth_boxes.numpy(), want[3]) and np.array_equal(hits.numpy(), want[4] != 0)


def test_engine_localize_matches_the_numpy_restatement(fake):
    E, lib = fake
    sizes = ((6, 10), (12, 17))
    planes, truth = _inputs(3, 2)
    thr = [0.9, 0.1, 0.4, 0.1, -0.25, 0.9, 1.5]                                    # unsorted, duplicated: as they come
    raw = L.raw_of(planes.numpy(), *sizes[1])
    for absolute in (False, True):
        _same(E.localize(planes, *sizes[1], thr, truth, absolute=absolute), L.restate(raw, thr, absolute, truth.numpy()))
    assert lib.calls[-1] == (3, 2, [float(np.float32(t)) for t in thr])
    got = E.localize(planes, *sizes[1], thr)                                      # no truth
    _same(got, L.restate(raw, thr, False))
    got = E.localize(planes, *sizes[1], truth=truth[0])                           # no thresholds, one [H, W] mask
    assert got[0].shape == (3, 0, 4) and got[4].shape == (3, 1) and lib.calls[-1] == (3, 1, [])
    _same(got, L.restate(raw, [], False, truth.numpy()[:1]))
    with pytest.raises(ValueError):
        E.localize(planes, *sizes[1], [0.1, float('nan')])
    with pytest.raises(ValueError):
        E.localize(planes, 12, 18, thr, truth)                                    # truth of another size: no resize here
    with pytest.raises(ValueError):
        E.localize(planes[:0], *sizes[1], thr)


@pytest.mark.parametrize('n_words,n_truth,n_thr', [(33, 2, 3), (2, 33, 3), (2, 1, 65), (33, 33, 65)])
def test_more_than_a_call_holds_runs_in_blocks(fake, n_words, n_truth, n_thr):
    E, lib = fake
    sizes = ((4, 6), (7, 9))
    planes, truth = _inputs(n_words, n_truth, sizes)
    thr = [float(t) for t in np.linspace(1.2, -0.2, n_thr)]
    got = E.localize(planes, *sizes[1], thr, truth)
    assert all(w <= 32 and g <= 32 and len(t) <= 64 for w, g, t in lib.calls)
    assert len(lib.calls) == -(-n_words // 32) * (-(-n_truth // 32) + -(-n_thr // 64) - 1)
    assert got[0].shape == (n_words, n_thr, 4) and got[3].shape == (n_truth, 4) and got[4].shape == (n_words, n_truth)
    _same(got, L.restate(L.raw_of(planes.numpy(), *sizes[1]), thr, False, truth.numpy()))


def test_mask_boxes_is_the_call_without_words(fake):
    from daam_amd import mask_boxes
    E, lib = fake
    stack = np.concatenate([S.truth_stack(33, 12, 17, seed=3), L.edge_truth(12, 17)])
    got = mask_boxes(torch.from_numpy(stack))
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), L.mask_boxes(stack))
    assert [c[:2] for c in lib.calls] == [(0, 32), (0, 3)] and got[-2].tolist() == [17, 12, -1, -1] and got[-1].tolist() == [16, 11, 16, 11]
    assert mask_boxes(torch.from_numpy(stack[3] != 0)).tolist() == [L.box_of(stack[3] != 0)]           # a bool [H, W] mask


class _Image:
    def __init__(self, width, height):
        self.size = (width, height)             # PIL order


PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


def _ghm(h=6, w=10):
    from daam_amd import GlobalHeatMap
    maps = torch.from_numpy(np.abs(np.random.default_rng(2).standard_normal((13, h, w))).astype(np.float32))
    return GlobalHeatMap(fd.FakeTokenizer(), PROMPT, maps)


def test_global_heat_map_localize_box_iou_and_pointing(fake):
    from daam_amd import Localization, Segmentation
    from daam_amd.utils import compute_token_merge_indices
    E, lib = fake
    ghm = _ghm()
    words = ['monkey', 'bicycle', ('photo', None)]
    truth_np = np.concatenate([S.truth_stack(2, 12, 17, seed=1), L.edge_truth(12, 17)[:1]])
    thr = [0.4, 0.9, 1.5, -0.25]
    loc = ghm.localize(words, _Image(17, 12), thr, torch.from_numpy(truth_np))     # rectangular maps: [image height, image width]
    assert isinstance(loc, Localization) and loc.words == ['monkey', 'bicycle', 'photo'] and loc.size == (12, 17)
    assert np.array_equal(loc.thresholds.numpy(), np.asarray(thr, np.float32))
    idx = [compute_token_merge_indices(ghm.tokenizer, PROMPT, *((w, None) if isinstance(w, str) else w))[0] for w in words]
    planes = torch.stack([ghm.heat_maps[i].mean(0) for i in idx]).numpy()
    want = L.restate(L.raw_of(planes, 12, 17), thr, False, truth_np)
    _same((loc.boxes, loc.peaks, loc.peak_values, loc.truth_boxes, loc.hits), want)
    assert loc.pointing() is loc.hits
    # box(): a tuple, None when empty, KeyError for a threshold that was not asked for
    assert loc.box('bicycle') == tuple(want[0][1, 0]) == loc.box(1, 0.4) and loc.box('monkey', 1.5) is None
    assert loc.box('photo', -0.25) == (0, 0, 16, 11)
    with pytest.raises(KeyError):
        loc.box('monkey', 0.41)
    with pytest.raises(KeyError):
        loc.box('cat')
    # box_iou against painting the boxes; the all-zero truth mask and the threshold 1.5 give empty boxes that score 0
    iou = loc.box_iou()
    assert iou.dtype == torch.float32 and iou.shape == (3, 3, 4)
    brute = np.array([[[L.box_iou(want[0][w, t], want[3][g]) for t in range(4)] for g in range(3)] for w in range(3)], np.float32)
    assert np.array_equal(iou.numpy(), brute) and (brute[:, 2] == 0).all() and (brute[:, :, 2] == 0).all() and brute.max() > 0
    mine = loc.box_iou([[0, 0, 16, 11], [3, 2, 3, 2]])
    assert (mine[:, 0, 3] == 1).all() and mine.shape == (3, 2, 4)
    # a Segmentation as truth, a square map's (size[0], size[1]) order, absolute, the default threshold; no truth
    seg = Segmentation(['a', 'b'], [], torch.from_numpy(S.truth_stack(2, 17, 12, seed=4)), None)
    sq = _ghm(8, 8).localize(['monkey'], _Image(17, 12), truth=seg, absolute=True)
    assert sq.boxes.shape == (1, 1, 4) and sq.hits.shape == (1, 2) and sq.size == (17, 12) and lib.calls[-1][2] == [float(np.float32(0.4))]
    none = ghm.localize(['monkey'], _Image(17, 12))
    assert none.truth_boxes is None and none.hits is None and np.array_equal(none.boxes.numpy(), want[0][:1, :1])
    with pytest.raises(ValueError):
        none.box_iou()
    with pytest.raises(ValueError):
        none.pointing()
    with pytest.raises(ValueError):
        ghm.localize([], _Image(17, 12))
    host = loc.cpu()
    assert host.words == loc.words and torch.equal(host.boxes, loc.boxes) and torch.equal(host.hits, loc.hits)


def test_localization_evaluator_against_a_hand_count():
    from daam_amd import Localization, LocalizationEvaluator
    thr = torch.tensor([0.2, 0.6], dtype=torch.float32)
    truth_boxes = torch.tensor([[0, 0, 9, 9], [10, 10, 19, 19]], dtype=torch.int32)

    def loc(boxes, hits):
        w = len(boxes)
        return Localization(['w%d' % i for i in range(w)], thr, (20, 20), torch.tensor(boxes, dtype=torch.int32), torch.zeros(w, 2, dtype=torch.int32),
                            torch.zeros(w, 3), truth_boxes, torch.tensor(hits))
    # word 0: the first truth box exactly at 0.2 (IoU 1), its left half at 0.6 (IoU 0.5: counts); word 1: empty at both
    first = loc([[[0, 0, 9, 9], [0, 0, 4, 9]], [[20, 20, -1, -1]] * 2], [[True, False], [False, False]])
    # word 0: 10 x 10 shifted by 5 against the second box (25 / 175) at 0.2, the second box at 0.6
    second = loc([[[15, 15, 24, 24], [10, 10, 19, 19]]], [[False, True]])
    ev = LocalizationEvaluator()
    assert ev.log(first) is ev and ev.log(second) is ev and len(ev) == 3
    assert ev.pointing_accuracy == pytest.approx(2 / 3) and ev.corloc.dtype == np.float32
    assert np.array_equal(ev.corloc, np.array([1 / 3, 2 / 3], np.float32)) and ev.best == (float(np.float32(0.6)), float(np.float32(2 / 3)))
    assert np.array_equal(np.stack(ev.ious), np.array([[1, 0.5], [0, 0], [25 / 175, 1]], np.float32))
    assert str(ev) == f'LocalizationEvaluator<{2 / 3:.4f} (pointing) {2 / 3:.4f} (CorLoc) at threshold 0.6, 2 thresholds, 3 samples>'
    pairs = LocalizationEvaluator('pairs').log(first, pairs=[(0, 1), (1, 0), (0, 0)])
    assert pairs.hits == [False, False, True] and np.array_equal(pairs.corloc, np.array([1 / 3, 1 / 3], np.float32))
    assert pairs.best == (float(np.float32(0.2)), float(np.float32(1 / 3)))                          # a tie: the lowest threshold
    with pytest.raises(ValueError):
        ev.log(Localization(['w'], thr[:1], (20, 20), torch.zeros(1, 1, 4, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32),
                            torch.zeros(1, 3), truth_boxes, torch.zeros(1, 2, dtype=torch.bool)))
    with pytest.raises(ValueError):
        LocalizationEvaluator().log(Localization(['w'], thr, (20, 20), torch.zeros(1, 2, 4, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32),
                                                 torch.zeros(1, 3), None, None))


# ---- the oracle alone: the GPU file's cases leave few pixels ambiguous ----------------------------------------------------------------
def test_oracle_cases_leave_few_pixels_ambiguous():
    """Every call ``test_gpu_localize.py::test_boxes_against_the_float64_oracle`` makes (``_sweep_domain.oracle_cases``, chosen for
    this cap): per word and threshold at most ``AMBIGUOUS_CAP`` of the pixels lie within the bound of the threshold, and no plane is
    ill-conditioned -- the inner and the outer box of the oracle differ by those pixels alone."""
    worst = 0.0
    for sizes, kinds, absolute, thr in S.oracle_cases():
        for kind, plane in zip(kinds, S.oracle_planes(sizes, kinds)):
            o = L.oracle_boxes(plane, *sizes[1], absolute, thr)
            assert not o['ill'], (sizes, kind, absolute)
            share = o['ambiguous'].reshape(len(thr), -1).mean(1)
            worst = max(worst, float(share.max()))
            assert (share <= D.AMBIGUOUS_CAP).all(), (sizes, kind, absolute, dict(zip(thr, share)))
            assert all(L.contains(out, inn) for out, inn in zip(o['outer'], o['inner']))
    print(f'largest ambiguous share {worst:.2e} (cap {D.AMBIGUOUS_CAP})')
