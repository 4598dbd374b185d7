"""The threshold sweep (``daam_threshold_sweep``, include/daam_eval.h) without a GPU: ``libdaam_eval.so`` builds beside
the other two libraries and exports what its header declares and the binding names; the header is C99; no kernel has scratch; every
argument the header rules out is refused before any HIP call; the Python layer (``engine.threshold_sweep``,
``GlobalHeatMap.threshold_sweep``, ``ThresholdSweep``, ``SweepEvaluator``) on a numpy stand-in of the library; and, on the float64
oracle alone, that the cases ``test_gpu_threshold_sweep.py`` holds to it leave few pixels ambiguous.  The kernels run in that file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _epilogue_domain as D
import _libcheck as LC
import _sweep_domain as S
from oracle import fake_diffusers as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('sweep_init_kernel', 'sweep_minmax_kernel', 'sweep_count_kernel', 'sweep_finalize_kernel')
E_INVALID = -1


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build(verbose=False)
    return build.EVAL_LIB


@pytest.fixture(scope='module')
def lib(built):
    from daam_amd import _native as nat
    return nat.load_eval()


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_library_builds_and_exports_its_header(built, lib):
    from daam_amd import _native as nat, build
    assert os.path.exists(built) and os.path.basename(built) == 'libdaam_eval.so' and not build.eval_stale()
    assert build.EVAL_SOURCES == ['daam_threshold_sweep.hip']
    exported = LC.exported(built)
    assert exported == LC.declared('daam_eval.h') == sorted(nat.EVAL_EXPORTS) and len(exported) == 4
    assert lib.daam_eval_abi_version() == 1 == nat.EVAL_ABI_VERSION
    assert len(lib.daam_threshold_sweep.argtypes) == 17
    assert nat.EVAL_LIB_PATH == built or os.environ.get('DAAM_EVAL_LIB')
    names = list(build.kernel_shas(built))
    assert sorted(sum(k in n for n in names) for k in KERNELS) == [1, 1, 1, 1] and len(names) == 4


def test_eval_header_is_c99(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "daam_eval.h"\nint main(void) { return DAAM_EVAL_ABI_VERSION == 1 && sizeof(&daam_threshold_sweep) ? 0 : 1; }\n')
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
    a = dict(word_maps=0x1000, n_words=3, h=16, w=24, out_h=37, out_w=53, absolute=0, thresholds=[0.1, 0.4, 0.9], truth=0x2000,
             n_truth=2, pred_area=0x3000, inter=0x4000, truth_area=0x5000, workspace=0x6000, workspace_bytes=None, stream=None)
    a.update(over)
    thr = a['thresholds']
    arr = None if thr is None else (ctypes.c_float * max(len(thr), 1))(*thr)
    n_thr = a.get('n_thr', 0 if thr is None else len(thr))
    if a['workspace_bytes'] is None:
        a['workspace_bytes'] = lib.daam_threshold_sweep_workspace(a['n_words'], a['n_truth'], n_thr, a['out_h'], a['out_w']) or 1 << 20
    rc = lib.daam_threshold_sweep(a['word_maps'], a['n_words'], a['h'], a['w'], a['out_h'], a['out_w'], a['absolute'], arr, n_thr,
                                  a['truth'], a['n_truth'], a['pred_area'], a['inter'], a['truth_area'], a['workspace'],
                                  a['workspace_bytes'], a['stream'])
    return rc, lib.daam_eval_last_error().decode()


BAD = {
    'NULL word_maps': dict(word_maps=None), 'NULL thresholds': dict(thresholds=None, n_thr=3), 'NULL pred_area': dict(pred_area=None),
    'NULL workspace': dict(workspace=None), 'NULL truth with masks': dict(truth=None), 'NULL inter with masks': dict(inter=None),
    'NULL truth_area with masks': dict(truth_area=None), 'truth without masks': dict(n_truth=0),
    'inter without masks': dict(n_truth=0, truth=None, truth_area=None), '0 words': dict(n_words=0), '33 words': dict(n_words=33),
    '33 truth masks': dict(n_truth=33), '-1 truth masks': dict(n_truth=-1), 'h 0': dict(h=0), 'w 129': dict(w=129), 'h 129': dict(h=129),
    'out_h 0': dict(out_h=0), 'out_w 0': dict(out_w=0), '2^31 pixels': dict(out_h=1 << 16, out_w=1 << 15),
    '0 thresholds': dict(thresholds=[], n_thr=0), '65 thresholds': dict(thresholds=[i / 65 for i in range(65)]),
    'unsorted': dict(thresholds=[0.1, 0.9, 0.4]), 'equal': dict(thresholds=[0.1, 0.4, 0.4]), 'nan': dict(thresholds=[0.1, float('nan'), 0.9]),
    'inf': dict(thresholds=[0.1, 0.4, float('inf')]), '-inf': dict(thresholds=[float('-inf'), 0.4, 0.9]),
    'small workspace': dict(workspace_bytes=256 + 4 * 3 * 4 * 3 - 1), 'unaligned workspace': dict(workspace=0x6002),
}


@pytest.mark.parametrize('what', sorted(BAD))
def test_out_of_range_is_refused_before_any_hip_call(lib, what):
    rc, msg = _call(lib, **BAD[what])
    assert rc == E_INVALID and msg, (what, rc, msg)


def test_workspace_is_monotone_and_zero_out_of_range(lib):
    ws = lib.daam_threshold_sweep_workspace
    assert ws(3, 2, 3, 37, 53) == 256 + 4 * 3 * 4 * 3
    for bad in ((0, 1, 1, 4, 4), (33, 1, 1, 4, 4), (1, -1, 1, 4, 4), (1, 33, 1, 4, 4), (1, 1, 0, 4, 4), (1, 1, 65, 4, 4), (1, 1, 1, 0, 4),
                (1, 1, 1, 4, 0), (1, 1, 1, 1 << 16, 1 << 15)):
        assert ws(*bad) == 0, bad
    assert ws(32, 32, 64, 46340, 46340) == 256 + 4 * 32 * 65 * 33
    grid = [(1, 2, 31, 32), (0, 1, 31, 32), (1, 2, 63, 64), (1, 37, 4096), (1, 53, 4096)]
    base = [g[0] for g in grid]
    for axis, values in enumerate(grid):
        sizes = [ws(*(base[:axis] + [v] + base[axis + 1:])) for v in values]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (axis, sizes)


# ---- the Python layer on the numpy stand-in -------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    return S.install(monkeypatch.setattr)


def _inputs(n_words, n_truth, sizes=((6, 10), (12, 17)), seed=5):
    planes = torch.from_numpy(S.word_planes(n_words, *sizes[0], seed=seed))
    truth = torch.from_numpy(S.truth_stack(n_truth, *sizes[1], seed=seed)) if n_truth else None
    return planes, truth


def _want(planes, sizes, thr, truth, absolute=False):
    return S.counts(S.values_of(planes.numpy(), *sizes[1], absolute), sorted(set(np.float32(t) for t in thr)), None if truth is None else truth.numpy())


def test_engine_sweep_matches_the_numpy_restatement(fake):
    E, lib = fake
    sizes = ((6, 10), (12, 17))
    planes, truth = _inputs(3, 2)
    thr = [i / 20 for i in range(21)]
    for absolute in (False, True):
        pred, inter, area = E.threshold_sweep(planes, *sizes[1], thr, truth, absolute=absolute)
        p, i, a = _want(planes, sizes, thr, truth, absolute)
        assert pred.dtype == inter.dtype == area.dtype == torch.int32
        assert (pred.numpy() == p).all() and (inter.numpy() == i).all() and (area.numpy() == a).all()
        assert (np.diff(pred.numpy(), axis=1) <= 0).all() and p[:, 0].max() > 0
    assert [c[:2] for c in lib.calls] == [(3, 2), (3, 2)]
    pred, inter, area = E.threshold_sweep(planes, *sizes[1], thr)                 # no truth: predicted areas only
    assert inter is None and area is None and (pred.numpy() == _want(planes, sizes, thr, None)[0]).all()
    with pytest.raises(ValueError):
        E.threshold_sweep(planes, *sizes[1], [])
    with pytest.raises(ValueError):
        E.threshold_sweep(planes, *sizes[1], [0.1, float('nan')])
    with pytest.raises(ValueError):
        E.threshold_sweep(planes, 12, 18, thr, truth)                             # truth of another size: no resize here


def test_thresholds_come_back_in_the_callers_order(fake):
    E, lib = fake
    sizes = ((6, 10), (12, 17))
    planes, truth = _inputs(2, 3)
    thr = [0.9, 0.1, 0.4, 0.1, -0.25, 0.9, 1.5, 0.4 + 1e-9]                        # unsorted, duplicated, equal as f32
    pred, inter, area = E.threshold_sweep(planes, *sizes[1], thr, truth)
    assert lib.calls[-1][2] == sorted(set(float(np.float32(t)) for t in thr)) and len(lib.calls[-1][2]) == 5
    for col, t in enumerate(thr):
        p, i, _ = _want(planes, sizes, [t], truth)
        assert (pred[:, col].numpy() == p[:, 0]).all() and (inter[:, :, col].numpy() == i[:, :, 0]).all()


@pytest.mark.parametrize('n_words,n_truth,n_thr', [(33, 2, 3), (2, 33, 3), (2, 1, 65), (33, 33, 65)])
def test_more_than_a_call_holds_runs_in_blocks(fake, n_words, n_truth, n_thr):
    E, lib = fake
    sizes = ((4, 6), (7, 9))
    planes, truth = _inputs(n_words, n_truth, sizes)
    thr = [float(t) for t in np.linspace(1.2, -0.2, n_thr)]                       # descending: the caller's order is kept
    pred, inter, area = E.threshold_sweep(planes, *sizes[1], thr, truth)
    assert all(w <= 32 and g <= 32 and len(t) <= 64 for w, g, t in lib.calls)
    assert len(lib.calls) == -(-n_words // 32) * -(-n_truth // 32) * -(-n_thr // 64)
    p, i, a = _want(planes, sizes, thr, truth)
    assert pred.shape == (n_words, n_thr) and inter.shape == (n_words, n_truth, n_thr) and area.shape == (n_truth,)
    assert (pred.numpy() == p[:, ::-1]).all() and (inter.numpy() == i[:, :, ::-1]).all() and (area.numpy() == a).all()


class _Image:
    def __init__(self, width, height):
        self.size = (width, height)             # PIL order


PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


def _ghm(h=6, w=10):
    from daam_amd import GlobalHeatMap
    maps = torch.from_numpy(np.abs(np.random.default_rng(2).standard_normal((13, h, w))).astype(np.float32))
    return GlobalHeatMap(fd.FakeTokenizer(), PROMPT, maps)


def test_global_heat_map_sweep_ratios_best_and_at(fake):
    from daam_amd import MaskOverlaps, Segmentation, ThresholdSweep
    from daam_amd.utils import compute_token_merge_indices
    E, lib = fake
    ghm = _ghm()
    words = ['monkey', 'bicycle', ('photo', None)]
    truth = torch.from_numpy(S.truth_stack(2, 12, 17, seed=1))
    sweep = ghm.threshold_sweep(words, _Image(17, 12), truth)                      # rectangular maps: [image height, image width]
    assert isinstance(sweep, ThresholdSweep) and sweep.words == ['monkey', 'bicycle', 'photo']
    assert np.array_equal(sweep.thresholds.numpy(), np.array([i / 20 for i in range(21)], np.float32))
    idx = [compute_token_merge_indices(ghm.tokenizer, PROMPT, *((w, None) if isinstance(w, str) else w))[0] for w in words]
    planes = torch.stack([ghm.heat_maps[i].mean(0) for i in idx])
    p, i, a = _want(planes, ((6, 10), (12, 17)), sweep.thresholds.numpy(), truth)
    assert (sweep.area_pred.numpy() == p).all() and (sweep.intersection.numpy() == i).all() and (sweep.area_truth.numpy() == a).all()
    # the ratios: numpy in f32, evaluate._ratios' operand order
    f = np.float32
    pf, inf_, af = p.astype(f)[:, None, :], i.astype(f), a.astype(f)[None, :, None]
    assert np.array_equal(sweep.iou().numpy(), inf_ / ((pf + af - inf_) + f(1e-8)))
    assert np.array_equal(sweep.ioa().numpy(), inf_ / (pf + f(1e-8))) and torch.equal(sweep.precision(), sweep.ioa())
    assert np.array_equal(sweep.recall().numpy(), inf_ / (af + f(1e-8)))
    # one column is the MaskOverlaps of that threshold, ratio for ratio
    col = sweep.at(0.4)
    assert isinstance(col, MaskOverlaps) and torch.equal(col.iou(), sweep.iou()[:, :, 8]) and torch.equal(col.ioa(), sweep.ioa()[:, :, 8])
    with pytest.raises(KeyError):
        sweep.at(0.41)
    iou = sweep.iou().numpy()
    thr, best = sweep.best('bicycle', 1)
    assert best == iou[1, 1].max() and thr == float(sweep.thresholds[int(iou[1, 1].argmax())]) and sweep.best(1, 1) == (thr, best)
    with pytest.raises(KeyError):
        sweep.best('cat')
    # a Segmentation as truth, thresholds of the caller, a square map's (size[0], size[1]) order, absolute
    seg = Segmentation(['a', 'b'], [], torch.from_numpy(S.truth_stack(2, 17, 12, seed=4)), None)
    sq = _ghm(8, 8).threshold_sweep(['monkey'], _Image(17, 12), seg, thresholds=[0.5, 0.2], absolute=True)
    assert sq.area_pred.shape == (1, 2) and sq.intersection.shape == (1, 2, 2) and lib.calls[-1][2] == [float(f(0.2)), 0.5]
    none = ghm.threshold_sweep(['monkey'], _Image(17, 12))
    assert none.intersection.shape == (1, 0, 21) and none.area_truth.shape == (0,) and (none.area_pred.numpy() == p[:1]).all()
    host = sweep.cpu()
    assert host.words == sweep.words and torch.equal(host.intersection, sweep.intersection)


def test_best_threshold_and_sweep_evaluator_follow_mean_evaluator(fake):
    """Per threshold, ``MeanEvaluator`` fed each word's best IoU over the truth masks: its ``mean_iou`` is the sweep's curve."""
    from daam_amd import MeanEvaluator, SweepEvaluator
    E, lib = fake
    ghm = _ghm()
    sweeps = [ghm.threshold_sweep(['monkey', 'bicycle', 'photo'], _Image(17, 12), torch.from_numpy(S.truth_stack(3, 12, 17, seed=s)))
              for s in (1, 2)]
    n_thr = 21
    per_thr = [MeanEvaluator() for _ in range(n_thr)]
    for sweep in sweeps:
        best = sweep.iou().numpy().max(1)                                          # [W, T]: the best candidate pairing
        for t in range(n_thr):
            per_thr[t].ious.extend(float(v) for v in best[:, t])
    # one image: best_threshold
    one = [MeanEvaluator() for _ in range(n_thr)]
    for t in range(n_thr):
        one[t].ious.extend(float(v) for v in sweeps[0].iou().numpy().max(1)[:, t])
    curve = np.array([m.mean_iou for m in one], np.float32)
    # f32 on the device against float64 on the host: two additions below 4 (2^-22 each) and a division
    assert np.abs(sweeps[0].mean_best_iou().numpy() - curve).max() <= 2.0 ** -21
    assert sweeps[0].best_threshold() == float(sweeps[0].thresholds[int(curve.argmax())])
    # many images
    ev = SweepEvaluator()
    for sweep in sweeps:
        assert ev.log(sweep) is ev
    want = np.array([m.mean_iou for m in per_thr], np.float32)
    assert len(ev) == 6 and ev.mean_iou.dtype == np.float32 and np.array_equal(ev.mean_iou, want)
    assert ev.best == (float(sweeps[0].thresholds[int(want.argmax())]), float(want.max()))
    assert str(ev) == f'SweepEvaluator<{want.max():.4f} (mIoU) at threshold {ev.best[0]:g}, 21 thresholds, 6 samples>'
    pairs = SweepEvaluator('pairs').log(sweeps[1], pairs=[(0, 2), (2, 0)])
    assert np.array_equal(pairs.mean_iou, np.array([np.mean([float(a), float(b)]) for a, b in
                                                    zip(sweeps[1].iou()[0, 2].numpy(), sweeps[1].iou()[2, 0].numpy())], np.float32))
    with pytest.raises(ValueError):
        ev.log(ghm.threshold_sweep(['monkey'], _Image(17, 12), torch.ones(12, 17, dtype=torch.uint8), thresholds=[0.3]))


# ---- the oracle alone: the GPU file's cases leave few pixels ambiguous ----------------------------------------------------------------
def test_oracle_cases_leave_few_pixels_ambiguous():
    """Every call ``test_gpu_threshold_sweep.py::test_counts_against_the_float64_oracle`` makes: per word and threshold at most
    ``AMBIGUOUS_CAP`` of the pixels lie within the bound of the threshold, and no min-max plane is ill-conditioned (the kinds
    ``_epilogue_domain.may_be_ill`` names are not among them).  The thresholds cover 0.0, 0.4, a negative one, 1.0 and 1.5."""
    seen, worst = set(), 0.0
    for sizes, kinds, absolute, thr in S.oracle_cases():
        assert not any(D.may_be_ill(sizes, k) for k in kinds) and set(kinds) <= set(D.MASK_KINDS)
        seen |= set(thr)
        for kind, plane in zip(kinds, S.oracle_planes(sizes, kinds)):
            o = S.oracle_intervals(plane, *sizes[1], absolute, thr)
            assert not o['ill'], (sizes, kind, absolute)
            share = o['ambiguous'].reshape(len(thr), -1).mean(1)
            worst = max(worst, float(share.max()))
            assert (share <= D.AMBIGUOUS_CAP).all(), (sizes, kind, absolute, dict(zip(thr, share)))
    assert {-0.25, 0.0, 0.4, 1.0, 1.5} <= seen
    print(f'largest ambiguous share {worst:.2e} (cap {D.AMBIGUOUS_CAP})')
