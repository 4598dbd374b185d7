"""``daam_threshold_sweep`` (include/daam_eval.h) on the device, through ctypes and through ``GlobalHeatMap``.

The sweep restates the arithmetic of ``daam_word_masks``, so against that route -- ``daam_word_masks(threshold=t)`` followed by
``daam_mask_overlap_matrix``, once per threshold -- every count is held to integer equality.  The test that does not lean on the
sibling kernel is ``test_counts_against_the_float64_oracle``: every count lies between the pixels ``_epilogue_domain.expand`` puts
surely above the threshold and those plus the ambiguous ones (``test_threshold_sweep_cpu.py`` caps how many those are)."""
import ctypes

import numpy as np
import pytest
import torch

import _epilogue_domain as D
import _sweep_domain as S
from oracle import fake_diffusers as fd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64                       # guard bytes on either side of a buffer


def _guarded(n_bytes, fill, offset=0):
    """A uint8 device buffer of ``n_bytes`` at ``offset`` bytes past 16-byte alignment, between two guards of 0xA5, filled with ``fill``."""
    raw = torch.full((GUARD + 16 + n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(raw.data_ptr() + GUARD) % 16) + offset
    raw[start:start + n_bytes] = fill
    return raw, start


def _guards_intact(raw, start, n_bytes):
    return bool((raw[:start] == 0xA5).all()) and bool((raw[start + n_bytes:] == 0xA5).all())


def sweep_raw(planes, out, thr, truth=None, absolute=False, truth_offset=0, ws_offset=0):
    """One ``daam_threshold_sweep`` call through ctypes on guarded buffers: outputs pre-filled with 0xFF, the truth stack at
    ``truth_offset`` bytes past alignment.  Returns int64 numpy ``(pred_area, inter, truth_area)`` after checking every guard."""
    from daam_amd import _native as nat
    lib = nat.load_eval()
    planes = torch.as_tensor(planes, dtype=torch.float32).to(DEV).contiguous()
    n, h, w = planes.shape
    g, t = (0 if truth is None else len(truth)), len(thr)
    oh, ow = out
    need = lib.daam_threshold_sweep_workspace(n, g, t, oh, ow)
    assert need > 0
    bufs = dict(pred=_guarded(4 * n * t, 0xFF), ws=_guarded(need, 0x5A, ws_offset))
    if g:
        bufs.update(inter=_guarded(4 * n * g * t, 0xFF), area=_guarded(4 * g, 0xFF), truth=_guarded(g * oh * ow, 0, truth_offset))
        raw, start = bufs['truth']
        raw[start:start + g * oh * ow] = torch.as_tensor(np.ascontiguousarray(truth), dtype=torch.uint8).to(DEV).reshape(-1)
        before = raw.clone()
    ptr = lambda k: bufs[k][0].data_ptr() + bufs[k][1] if k in bufs else None
    nat.check_eval(lib.daam_threshold_sweep(planes.data_ptr(), n, h, w, oh, ow, 1 if absolute else 0, (ctypes.c_float * t)(*thr), t,
                                            ptr('truth'), g, ptr('pred'), ptr('inter'), ptr('area'), ptr('ws'), need,
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    sizes = dict(pred=4 * n * t, ws=need, inter=4 * n * g * t, area=4 * g, truth=g * oh * ow)
    for k, (raw, start) in bufs.items():
        assert _guards_intact(raw, start, sizes[k]), f'guard bytes around {k} changed'
    if g:
        assert torch.equal(bufs['truth'][0], before), 'the truth bytes changed'

    def ints(k, shape):
        raw, start = bufs[k]
        return raw[start:start + sizes[k]].cpu().numpy().view(np.uint32).astype(np.int64).reshape(shape)
    return ints('pred', (n, t)), ints('inter', (n, g, t)) if g else None, ints('area', (g,)) if g else None


def route(planes, out, thr, truth=None, absolute=False):
    """The existing route, once per threshold: ``daam_word_masks`` then ``daam_mask_overlap_matrix`` -- int64 numpy counts."""
    from daam_amd import engine as E, evaluate as ev
    planes = torch.as_tensor(planes, dtype=torch.float32).to(DEV).contiguous()
    masks_t = None if truth is None else torch.as_tensor(np.ascontiguousarray(truth)).to(DEV)
    pred, inter, area = [], [], None
    for t in thr:
        _, masks, _ = E.word_masks(planes, [[j] for j in range(planes.shape[0])], out[0], out[1], absolute=absolute, threshold=float(t),
                                   labels=False)
        ov = ev.mask_overlap_matrix(masks, masks_t)
        pred.append(ov.area_a.cpu().numpy().astype(np.int64))
        if truth is not None:
            inter.append(ov.intersection.cpu().numpy().astype(np.int64))
            area = ov.area_b.cpu().numpy().astype(np.int64)
    return np.stack(pred, 1), (np.stack(inter, 2) if truth is not None else None), area


def _assert_same(got, want, what):
    for name, a, b in zip(('pred_area', 'inter', 'truth_area'), got, want):
        assert (a is None) == (b is None), (what, name)
        if a is not None:
            assert a.shape == b.shape and (a == b).all(), f'{what}: {name} differs at {int((a != b).sum())} of {a.size} counts'


# ---- exact against the existing route ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('combo', S.COMBOS, ids=lambda c: 'W%d-G%d-T%d' % c)
@pytest.mark.parametrize('absolute', [False, True], ids=['minmax', 'absolute'])
@pytest.mark.parametrize('sizes', S.SIZES, ids=lambda s: '%dx%d-%dx%d' % (s[0] + s[1]))
def test_counts_equal_the_existing_route(sizes, absolute, combo):
    n_words, n_truth, n_thr = combo
    planes = S.word_planes(n_words, *sizes[0], seed=n_thr)
    truth = S.truth_stack(n_truth, *sizes[1], seed=n_words) if n_truth else None
    thr = S.thresholds(n_thr)
    got = sweep_raw(planes, sizes[1], thr, truth, absolute)
    _assert_same(got, route(planes, sizes[1], thr, truth, absolute), (sizes, absolute, combo))
    assert (np.diff(got[0], axis=1) <= 0).all()


def test_the_full_call_equals_the_existing_route():
    """32 words x 32 truth masks x 64 thresholds: more counters than the LDS holds, the workgroup takes the words in groups."""
    sizes = S.FULL_SIZE
    planes, truth, thr = S.word_planes(32, *sizes[0], seed=9), S.truth_stack(32, *sizes[1], seed=9), S.thresholds(64)
    assert {np.float32(t) for t in (-0.25, 0.0, 0.4, 1.0, 1.5)} <= {np.float32(t) for t in thr}
    for absolute in (False, True):
        _assert_same(sweep_raw(planes, sizes[1], thr, truth, absolute), route(planes, sizes[1], thr, truth, absolute), ('full', absolute))


# ---- the float64 oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(S.oracle_cases()), ids=lambda c: '%dx%d-%dx%d-%s-%s' % (c[0][0] + c[0][1] + (c[1][0], 'abs' if c[2] else 'minmax')))
def test_counts_against_the_float64_oracle(case):
    sizes, kinds, absolute, thr = case
    planes = S.oracle_planes(sizes, kinds)
    truth = S.truth_stack(3, *sizes[1], seed=21)
    pred, inter, area = sweep_raw(planes, sizes[1], thr, truth, absolute)
    assert (area == (truth != 0).sum((1, 2))).all()
    for j, plane in enumerate(planes):
        o = S.oracle_intervals(plane, *sizes[1], absolute, thr)
        assert not o['ill']
        sure, amb = o['sure'].sum((1, 2)), o['ambiguous'].sum((1, 2))
        print(f'{sizes} {kinds[j]} absolute={absolute}: pred {pred[j].tolist()} sure {sure.tolist()} ambiguous {amb.tolist()}')
        assert (pred[j] >= sure).all() and (pred[j] <= sure + amb).all(), (kinds[j], pred[j], sure, amb)
        for g in range(len(truth)):
            s = (o['sure'] & (truth[g] != 0)).sum((1, 2))
            a = (o['ambiguous'] & (truth[g] != 0)).sum((1, 2))
            assert (inter[j, g] >= s).all() and (inter[j, g] <= s + a).all(), (kinds[j], g, inter[j, g], s, a)


# ---- truth bytes ------------------------------------------------------------------------------------------------------------------------
def test_truth_bytes_at_any_alignment_count_once():
    """A stack at an odd byte offset with an odd plane size (37 x 53 = 1961); the set bytes are 1, 2, 128 and 255."""
    sizes = S.FULL_SIZE
    planes, thr = S.word_planes(3, *sizes[0], seed=2), S.thresholds(21)
    truth = S.truth_stack(5, *sizes[1], seed=4)
    assert {1, 2, 128, 255} <= set(np.unique(truth)) and truth[0].size % 2 == 1
    want = S.counts(np.zeros((1,) + sizes[1]), [-1.0], truth)[2]
    ones = (truth != 0).astype(np.uint8)
    base = sweep_raw(planes, sizes[1], thr, ones)
    for offset in (1, 3, 7):
        got = sweep_raw(planes, sizes[1], thr, truth, truth_offset=offset)
        _assert_same(got, base, f'offset {offset}')
        assert (got[2] == want).all()
    _assert_same(sweep_raw(planes, sizes[1], thr, truth, ws_offset=4), base, 'workspace 4 bytes past alignment')


# ---- independence -----------------------------------------------------------------------------------------------------------------------
def test_counts_do_not_depend_on_the_rest_of_the_call():
    sizes = ((64, 64), (200, 333))
    planes, truth, thr = S.word_planes(32, *sizes[0], seed=1), S.truth_stack(5, *sizes[1], seed=1), S.thresholds(21)
    full = sweep_raw(planes, sizes[1], thr, truth)
    _assert_same(sweep_raw(planes, sizes[1], thr, truth), full, 'a second run')
    for j in (0, 13, 31):                                          # a word alone
        alone = sweep_raw(planes[j:j + 1], sizes[1], thr, truth)
        assert (alone[0][0] == full[0][j]).all() and (alone[1][0] == full[1][j]).all() and (alone[2] == full[2]).all()
    pick = [0, 3, 8, 20]                                           # a subset of the thresholds: the same columns
    sub = sweep_raw(planes, sizes[1], [thr[i] for i in pick], truth)
    assert (sub[0] == full[0][:, pick]).all() and (sub[1] == full[1][:, :, pick]).all() and (sub[2] == full[2]).all()
    none = sweep_raw(planes, sizes[1], thr, None)                   # no truth masks: the same predicted areas
    assert none[1] is None and none[2] is None and (none[0] == full[0]).all()
    one = sweep_raw(planes, sizes[1], thr, truth[2:3])              # a truth mask alone
    assert (one[1][:, 0] == full[1][:, 2]).all() and (one[0] == full[0]).all()


# ---- invariants -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('absolute', [False, True])
def test_invariants(absolute):
    sizes = ((24, 16), (16, 24))
    planes, thr = S.word_planes(7, *sizes[0], seed=6), S.thresholds(64)
    # disjoint truth masks that tile the image: pixel p belongs to mask p % 5
    tiles = np.stack([(np.arange(16 * 24).reshape(16, 24) % 5 == g) for g in range(5)]).astype(np.uint8) * 255
    pred, inter, area = sweep_raw(planes, sizes[1], thr, tiles, absolute)
    assert (np.diff(pred, axis=1) <= 0).all() and (np.diff(inter, axis=2) <= 0).all()
    assert (inter <= pred[:, None, :]).all() and (inter <= area[None, :, None]).all()
    assert (inter.sum(1) == pred).all() and area.sum() == 16 * 24
    assert (pred[:, 0] == 16 * 24).all() if not absolute else True          # min-max values are >= 0 > -0.25


def test_single_pixel_and_constant_plane():
    """``absolute=False`` makes both exactly 0: nothing above a threshold >= 0, every pixel above a negative one."""
    thr = [-0.25, 0.0, 0.4]
    # a single output pixel; a constant plane copied at its own size; a plane of zeros resized (0 x weight is 0 in every pixel --
    # any other constant is resized to weight sums that differ in the last bit, the ill-conditioned kind of _epilogue_domain)
    for planes, out in ((S.word_planes(2, 8, 8, seed=3), (1, 1)), (np.full((2, 5, 7), 0.25, np.float32), (5, 7)),
                        (np.zeros((2, 5, 7), np.float32), (9, 11))):
        n = out[0] * out[1]
        truth = np.ones((1,) + out, np.uint8)
        pred, inter, area = sweep_raw(planes, out, thr, truth)
        assert (pred == [[n, 0, 0]] * len(planes)).all() and (inter[:, 0] == pred).all() and area[0] == n


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


def test_global_heat_map_sweep_equals_segment():
    ghm = _ghm(16, 24)
    words, image = ['monkey', 'bicycle', ('photo', None)], _Image(53, 37)
    truth = torch.from_numpy(S.truth_stack(4, 37, 53, seed=8)).to(DEV)
    sweep = ghm.threshold_sweep(words, image, truth)
    assert sweep.intersection.is_cuda and sweep.intersection.dtype == torch.int32 and sweep.intersection.shape == (3, 4, 21)
    iou, ioa = sweep.iou(), sweep.ioa()
    for t in (2, 8, 15):
        seg = ghm.segment(words, image, threshold=t / 20, labels=False)
        assert torch.equal(iou[..., t], seg.iou(truth)) and torch.equal(ioa[..., t], seg.ioa(truth))
        ov = seg.overlaps(truth)
        assert torch.equal(sweep.at(t / 20).intersection, ov.intersection) and torch.equal(sweep.area_pred[:, t], ov.area_a)
        assert torch.equal(sweep.area_truth, ov.area_b)
    as_seg = ghm.threshold_sweep(words, image, ghm.segment(['riding', 'a'], image, labels=False), thresholds=[0.5, 0.3], absolute=True)
    assert as_seg.intersection.shape == (3, 2, 2)


def test_best_agrees_with_a_brute_force_sweep_of_segment():
    from daam_amd import SweepEvaluator
    ghm = _ghm(64, 64)
    words, image = ['monkey', 'bicycle'], _Image(128, 128)
    truth = ghm.segment(['monkey', 'riding'], image, threshold=0.45, labels=False).masks
    thr = [i / 20 for i in range(21)]
    sweep = ghm.threshold_sweep(words, image, truth)
    brute = torch.stack([ghm.segment(words, image, threshold=t, labels=False).iou(truth) for t in thr], dim=2).cpu().numpy()
    assert np.array_equal(sweep.iou().cpu().numpy(), brute)
    for w, word in enumerate(words):
        for g in range(2):
            t = int(brute[w, g].argmax())
            assert sweep.best(word, g) == (float(np.float32(thr[t])), float(brute[w, g, t]))
    assert sweep.best('monkey', 0)[1] > 0.9 and abs(sweep.best('monkey', 0)[0] - 0.45) < 1e-6      # the mask it was cut from
    curve = brute.max(1).mean(0)
    assert sweep.best_threshold() == float(np.float32(thr[int(curve.argmax())]))
    ev = SweepEvaluator().log(sweep)
    assert len(ev) == 2 and np.array_equal(ev.mean_iou, np.array([np.mean(c) for c in brute.max(1).astype(np.float64).T], np.float32))
