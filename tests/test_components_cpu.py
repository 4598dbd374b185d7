"""Connected components (``daam_mask_components``, include/daam_components.h) without a GPU:
``libdaam_components.so`` builds beside the other libraries and exports what its header declares and the binding names; the header
is C99; no kernel has scratch; every argument the header rules out is refused before any HIP call; the numpy reference against a
breadth-first labeller and ``scipy.ndimage``; the kernels' union rules, restated pixel by pixel, close to the reference's
components; and the Python layer (``engine.mask_components``, ``MaskComponents``, ``Segmentation.components`` / ``clean``,
``GlobalHeatMap.localize(component='largest')``, ``LocalizationEvaluator``) on a numpy stand-in of the library.  The kernels run in
``test_gpu_components.py``."""
import os
import subprocess

import numpy as np
import pytest
import torch

import _components_domain as C
import _libcheck as LC
import _locate_domain as L
from oracle import fake_diffusers as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ('comp_init_kernel', 'comp_local_kernel', 'comp_seam_kernel', 'comp_flatten_kernel', 'comp_scan_kernel', 'comp_roots_kernel',
           'comp_output_kernel')
E_INVALID = -1


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build(verbose=False)
    return build.COMPONENTS_LIB


@pytest.fixture(scope='module')
def lib(built):
    from daam_amd import _native as nat
    return nat.load_components()


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_library_builds_and_exports_its_header(built, lib):
    from daam_amd import _native as nat, build
    assert os.path.exists(built) and os.path.basename(built) == 'libdaam_components.so' and not build.components_stale()
    assert build.COMPONENTS_SOURCES == ['daam_components.hip']
    exported = LC.exported(built)
    assert exported == LC.declared('daam_components.h') == sorted(nat.COMPONENTS_EXPORTS) and len(exported) == 4
    assert lib.daam_components_abi_version() == 1 == nat.COMPONENTS_ABI_VERSION
    assert len(lib.daam_mask_components.argtypes) == 16
    assert nat.COMPONENTS_LIB_PATH == built or os.environ.get('DAAM_COMPONENTS_LIB')
    names = list(build.kernel_shas(built))
    assert sorted(sum(k in n for n in names) for k in KERNELS) == [1] * len(KERNELS) and len(names) == len(KERNELS)


def test_components_header_is_c99(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "daam_components.h"\nint main(void) { return DAAM_COMPONENTS_ABI_VERSION == 1 && sizeof(&daam_mask_components) ? 0 : 1; }\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o',
                    str(tmp_path / 'use.o')], check=True)


def test_no_kernel_has_scratch(built):
    """Private segment size 0 and the private-segment enable bit clear in every kernel descriptor."""
    from daam_amd import build
    names = list(build.kernel_shas(built))
    assert len(names) == len(KERNELS)
    LC.assert_no_scratch(built, names)


# ---- argument checks: all of them before any HIP call, so they run here ---------------------------------------------------------------
def _call(lib, **over):
    """A call that is in range but for ``over``; pointers are small fake addresses (nothing is dereferenced)."""
    a = dict(masks=0x1000, n_masks=3, h=37, w=53, connectivity=8, min_area=0, keep=1, max_comp=16, labels=0x2000, counts=0x3000,
             comps=0x4000, largest=0x5000, kept=0x7000, workspace=0x6000, workspace_bytes=None, stream=None)
    a.update(over)
    if a['workspace_bytes'] is None:
        a['workspace_bytes'] = lib.daam_mask_components_workspace(a['n_masks'], a['h'], a['w'], a['max_comp']) or 1 << 20
    rc = lib.daam_mask_components(a['masks'], a['n_masks'], a['h'], a['w'], a['connectivity'], a['min_area'], a['keep'], a['max_comp'],
                                  a['labels'], a['counts'], a['comps'], a['largest'], a['kept'], a['workspace'], a['workspace_bytes'],
                                  a['stream'])
    return rc, lib.daam_components_last_error().decode()


BAD = {
    'connectivity 5': dict(connectivity=5), 'connectivity 0': dict(connectivity=0), 'keep 3': dict(keep=3), 'keep -1': dict(keep=-1),
    '33 masks': dict(n_masks=33), '-1 masks': dict(n_masks=-1), 'h 0': dict(h=0), 'w 0': dict(w=0), '2^31 pixels': dict(h=1 << 16, w=1 << 15),
    'min_area -1': dict(min_area=-1), 'max_comp -1': dict(max_comp=-1), 'max_comp 65537': dict(max_comp=65537),
    'NULL masks': dict(masks=None), 'NULL counts': dict(counts=None), 'NULL largest': dict(largest=None), 'NULL comps': dict(comps=None),
    'comps without rows': dict(max_comp=0), 'NULL kept': dict(kept=None), 'kept without keep': dict(keep=0),
    'NULL workspace': dict(workspace=None), 'small workspace': dict(workspace_bytes=512 + 2 * 8 * ((4 * 3 * 37 * 53 + 7) // 8) + 4 * 3 * 37 - 1),
    'unaligned workspace': dict(workspace=0x6004),
}


@pytest.mark.parametrize('what', sorted(BAD))
def test_out_of_range_is_refused_before_any_hip_call(lib, what):
    rc, msg = _call(lib, **BAD[what])
    assert rc == E_INVALID and msg, (what, rc, msg)


def test_a_call_without_masks_launches_nothing(lib):
    assert _call(lib, n_masks=0) == (0, _call(lib, n_masks=0)[1]) and _call(lib, n_masks=0, labels=None)[0] == 0


def test_workspace_is_monotone_and_zero_out_of_range(lib):
    ws = lib.daam_mask_components_workspace
    fake = C.FakeComponentsLib().daam_mask_components_workspace
    assert ws(3, 37, 53, 16) == 512 + 2 * 8 * ((4 * 3 * 37 * 53 + 7) // 8) + 8 * ((4 * 3 * 37 + 7) // 8) == fake(3, 37, 53, 16)
    assert ws(0, 4, 4, 0) == 512 and ws(1, 1, 1, 0) == 512 + 24 == fake(1, 1, 1, 0) and ws(32, 1024, 1024, 256) == fake(32, 1024, 1024, 256)
    for bad in ((33, 4, 4, 1), (-1, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 1 << 16, 1 << 15, 1), (1, 4, 4, -1), (1, 4, 4, 65537)):
        assert ws(*bad) == 0, bad
    assert ws(32, (1 << 31) - 1, 1, 65536) == 512 + 3 * 4 * 32 * ((1 << 31) - 1) and ws(32, 46340, 46340, 0) > 8 * 32 * 46340 * 46340
    grid = [(1, 2, 31, 32), (1, 37, 4096), (1, 53, 256, 257, 4096), (0, 1, 256, 65536)]
    base = [g[0] for g in grid]
    for axis, values in enumerate(grid):
        sizes = [ws(*(base[:axis] + [v] + base[axis + 1:])) for v in values]
        assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes), (axis, sizes)


# ---- the reference, and the union rules ------------------------------------------------------------------------------------------------
SMALL = [(name, hw) for name in ('spiral', 'comb', 'checker', 'noise', 'dense', 'blobs', 'full', 'empty') for hw in ((52, 76), (1, 37), (37, 1), (1, 1))]
SEAMED = [(name, C.SEAMS) for name in C.SEAM_MASKS]


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('name,hw', SMALL + [(n, hw) for n, hw in SEAMED if n in ('u', 'ties', 'corners', 'ring')], ids=lambda v: str(v))
def test_reference_equals_breadth_first_search(name, hw, connectivity):
    mask = C.SEAM_MASKS[name](*hw)
    got, want = C.label(mask, connectivity), C.label_bfs(mask, connectivity)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), (name, hw)


@pytest.mark.parametrize('connectivity', [4, 8])
def test_reference_equals_scipy(connectivity):
    ndimage = pytest.importorskip('scipy.ndimage')
    structure = ndimage.generate_binary_structure(2, 1 if connectivity == 4 else 2)
    for name, hw in SMALL + SEAMED + [('blobs', (300, 700))]:
        mask = C.SEAM_MASKS[name](*hw)
        labels, roots, areas, boxes = C.label(mask, connectivity)
        theirs, k = ndimage.label(mask, structure)
        assert k == len(roots) and np.array_equal(labels, theirs.astype(np.int32) - 1), (name, hw)
        found = ndimage.find_objects(theirs)
        assert [[s[1].start, s[0].start, s[1].stop - 1, s[0].stop - 1] for s in found] == boxes.tolist(), (name, hw)
        assert np.array_equal(areas, np.bincount(theirs.ravel())[1:])


def test_the_hand_made_masks_are_what_they_are_for():
    r4, r8 = C.reference(C.checkerboard(52, 76)[None], 4, max_comp=4), C.reference(C.checkerboard(52, 76)[None], 8, max_comp=4)
    assert r4['counts'].tolist() == [[52 * 76 // 2] * 2] and r8['counts'].tolist() == [[1, 1]] and r4['comps'][0, :, 0].tolist() == [0, 2, 4, 6]
    for name in ('spiral', 'comb', 'comb_top'):
        assert all(C.reference(C.SEAM_MASKS[name](*C.SEAMS)[None], c)['counts'][0, 0] == 1 for c in (4, 8)), name
    u = C.reference(C.u_shape(*C.SEAMS)[None], 4)
    assert u['counts'][0, 0] == 2 and u['comps'][0, 0, 0] == 3 * 531 + 200 and u['labels'][0, 5, 10] == 0      # the right arm's top is the root
    assert C.reference(C.ring_and_blob(*C.SEAMS)[None], 8)['counts'][0, 0] == 2
    assert [C.reference(C.corner_diagonals(*C.SEAMS)[None], c)['counts'][0, 0] for c in (4, 8)] == [4, 2]
    ties = C.reference(C.equal_areas(*C.SEAMS)[None], 8, min_area=6, keep=2)
    assert ties['comps'][0, :3, 1].tolist() == [6, 6, 5] and ties['largest'][0].tolist() == [532, 6, 1, 1, 3, 2] and ties['counts'].tolist() == [[3, 2]]
    assert ties['kept'].sum() == 6 and ties['kept'][0, 1:3, 1:4].all()
    empty = C.reference(np.zeros((1, 5, 7), np.uint8), 8, keep=2)
    assert empty['largest'].tolist() == [[-1, 0, 7, 5, -1, -1]] and not empty['kept'].any() and (empty['comps'] == C.sentinel(5, 7)).all()


@pytest.mark.parametrize('connectivity', [4, 8])
@pytest.mark.parametrize('name', sorted(C.SEAM_MASKS))
def test_the_kernels_union_rules_close_to_the_components(name, connectivity):
    """The unions of the local kernel (inside a tile) and of the seam kernel (across tiles), made in any order, give the
    reference's components -- and the seam kernel's are needed wherever a component crosses a tile edge."""
    mask = C.SEAM_MASKS[name](*C.SEAMS)
    local, seam = C.rule_unions(mask, connectivity)
    want = C.label(mask, connectivity)[0]
    assert np.array_equal(C.closure_labels(mask, local + seam), want)
    assert np.array_equal(C.closure_labels(mask, seam[::-1] + local[::-1]), want)
    if name in ('spiral', 'comb', 'u', 'ring', 'full') or (name == 'corners' and connectivity == 8):
        assert seam and not np.array_equal(C.closure_labels(mask, local), want)


# ---- the Python layer on the numpy stand-in -------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    return C.install(monkeypatch.setattr)


def _stack(n, h=20, w=31):
    return np.stack([C.blobs(h, w, seed=i, n=3, speckle=0.02) for i in range(n)])


@pytest.mark.parametrize('n', [1, 33, 65])
def test_engine_mask_components_runs_in_blocks_of_32(fake, n):
    E, lib, _, _ = fake
    stack = _stack(n)
    got = E.mask_components(torch.from_numpy(stack), connectivity=4, min_area=3, keep='area', max_components=5)
    want = C.reference(stack, 4, 3, 1, 5)
    assert [c[0] for c in lib.calls] == [32] * (n // 32) + [n % 32] and all(c[1:] == (4, 3, 1, 5, True) for c in lib.calls)
    assert [t.dtype for t in got] == [torch.int32] * 4 + [torch.uint8]
    assert all(np.array_equal(t.numpy(), want[k]) for t, k in zip(got, ('labels', 'counts', 'comps', 'largest', 'kept')))
    none = E.mask_components(torch.from_numpy(stack[0] != 0), keep=None, max_components=0, labels=False)         # a bool [H, W] mask
    assert none[0] is None and none[4] is None and none[2].shape == (1, 0, 6) and lib.calls[-1] == (1, 8, 0, 0, 0, False)
    assert np.array_equal(none[3].numpy(), C.reference(stack[:1], 8)['largest'])
    for bad in (dict(connectivity=6), dict(keep='all'), dict(min_area=-1), dict(max_components=65537)):
        with pytest.raises(ValueError):
            E.mask_components(torch.from_numpy(stack), **bad)


def test_mask_components_dataclass(fake):
    from daam_amd import MaskComponents, mask_components
    stack = np.concatenate([_stack(2), np.zeros((1, 20, 31), np.uint8), C.checkerboard(20, 31)[None]])
    mc = mask_components(torch.from_numpy(stack), connectivity=4, max_components=8, keep='largest')
    want = C.reference(stack, 4, 0, 2, 8)
    assert isinstance(mc, MaskComponents) and [mc.n(m) for m in range(4)] == want['counts'][:, 0].tolist() and mc.n(3) == 310 and mc.n(2) == 0
    for m in range(4):
        k = min(mc.n(m), 8)
        assert np.array_equal(mc.areas(m).numpy(), want['comps'][m, :k, 1]) and np.array_equal(mc.boxes(m).numpy(), want['comps'][m, :k, 2:])
        assert mc.boxes(m).shape == (k, 4)
    boxes = mc.largest_boxes()
    assert boxes.dtype == torch.int32 and boxes.shape == (4, 4) and boxes[2].tolist() == [31, 20, -1, -1] == L.box_of(stack[2] != 0)
    assert np.array_equal(boxes.numpy(), want['largest'][:, 2:]) and np.array_equal(mc.kept.numpy(), want['kept'])
    host = mc.cpu()
    assert torch.equal(host.labels, mc.labels) and torch.equal(host.largest, mc.largest) and mask_components(torch.from_numpy(stack), labels=False).cpu().labels is None


def test_segmentation_components_and_clean(fake):
    from daam_amd import Segmentation, WordHeatMap
    E, lib, _, _ = fake
    stack = _stack(3)
    heat = [WordHeatMap(torch.zeros(4, 4), w, None) for w in 'abc']
    seg = Segmentation(['a', 'b', 'c'], heat, torch.from_numpy(stack), torch.zeros(20, 31, dtype=torch.uint8))
    mc = seg.components(connectivity=4, min_area=4)
    assert np.array_equal(mc.counts.numpy(), C.reference(stack, 4, 4)['counts']) and lib.calls[-1] == (3, 4, 4, 0, 256, True)
    clean = seg.clean(min_area=4)
    assert clean.words == seg.words and clean.word_heat_maps == heat and clean.labels is None and clean.masks.dtype == torch.uint8
    assert np.array_equal(clean.masks.numpy(), C.reference(stack, 8, 4, 1)['kept']) and lib.calls[-1] == (3, 8, 4, 1, 0, False)
    big = seg.clean(largest=True, connectivity=4)
    want = C.reference(stack, 4, 0, 2)
    assert np.array_equal(big.masks.numpy(), want['kept']) and lib.calls[-1] == (3, 4, 0, 2, 0, False)
    bar = int(np.sort(want['largest'][:, 1])[1])                                # the middle one of the three largest areas
    gated = seg.clean(min_area=bar + 1, largest=True, connectivity=4).masks.numpy()
    assert [bool(g.any()) for g in gated] == [a > bar for a in want['largest'][:, 1]] and sum(bool(g.any()) for g in gated) < 3
    assert all(np.array_equal(g, k) for g, k, a in zip(gated, want['kept'], want['largest'][:, 1]) if a > bar)


class _Image:
    def __init__(self, width, height):
        self.size = (width, height)             # PIL order


PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


def _ghm(h=6, w=10):
    from daam_amd import GlobalHeatMap
    maps = torch.from_numpy(np.abs(np.random.default_rng(2).standard_normal((13, h, w))).astype(np.float32))
    return GlobalHeatMap(fd.FakeTokenizer(), PROMPT, maps)


def test_localize_largest_component_and_the_untouched_default(fake):
    E, lib, locate, word_mask_calls = fake
    ghm, image = _ghm(), _Image(17, 12)
    words, thr = ['monkey', 'bicycle', ('photo', None)], [0.4, 0.7, 1.5]
    truth = torch.from_numpy(L.edge_truth(12, 17))
    plain = ghm.localize(words, image, thr, truth)
    assert locate.calls == [(3, 2, [float(np.float32(t)) for t in thr])] and not lib.calls and not word_mask_calls     # as before this existed
    loc = ghm.localize(words, image, thr, truth, component='largest', connectivity=4)
    assert locate.calls[1:] == [(3, 2, [])] and word_mask_calls == [float(np.float32(t)) for t in thr]
    assert lib.calls == [(3, 4, 0, 0, 0, False)] * 3
    assert loc.boxes.shape == (3, 3, 4) and loc.boxes.dtype == torch.int32 and torch.equal(loc.thresholds, plain.thresholds)
    for k in ('peaks', 'peak_values', 'truth_boxes', 'hits'):
        assert torch.equal(getattr(loc, k), getattr(plain, k)), k
    assert loc.words == plain.words and loc.size == plain.size == (12, 17)
    differs = 0
    for t, tau in enumerate(thr):
        masks = ghm.segment(words, image, threshold=tau, labels=False).masks.numpy()
        want = C.reference(masks, 4)['largest'][:, 2:]
        assert np.array_equal(loc.boxes[:, t].numpy(), want) and np.array_equal(plain.boxes[:, t].numpy(), L.mask_boxes(masks))
        differs += int((want != L.mask_boxes(masks)).any())
    assert differs and loc.boxes[:, 2].tolist() == [[17, 12, -1, -1]] * 3          # noisy planes: speckles move the whole-mask box; 1.5: empty
    assert loc.box_iou().shape == (3, 2, 3) and loc.box('monkey', 1.5) is None
    assert ghm.localize(words, image, [], component='largest').boxes.shape == (3, 0, 4)
    with pytest.raises(ValueError):
        ghm.localize(words, image, thr, component='all')


def test_a_speckle_turns_a_corloc_miss_into_a_hit(fake):
    """One word on a 20 x 20 image: a 10 x 10 blob on the truth box and one stray pixel in the far corner.  The whole-mask box is
    the image (IoU 100 / 400: a miss), the largest component's box is the truth box (IoU 1: a hit)."""
    from daam_amd import Localization, LocalizationEvaluator, mask_components
    mask = np.zeros((1, 20, 20), np.uint8)
    mask[0, :10, :10] = 1
    mask[0, 19, 19] = 1
    truth_boxes = torch.tensor([[0, 0, 9, 9]], dtype=torch.int32)
    thr = torch.tensor([0.4], dtype=torch.float32)

    def corloc(boxes):
        loc = Localization(['dog'], thr, (20, 20), boxes.reshape(1, 1, 4), torch.zeros(1, 2, dtype=torch.int32), torch.zeros(1, 3), truth_boxes,
                           torch.ones(1, 1, dtype=torch.bool))
        ev = LocalizationEvaluator().log(loc)
        return float(ev.corloc[0]), float(np.stack(ev.ious)[0, 0])
    assert corloc(torch.tensor(L.mask_boxes(mask), dtype=torch.int32)) == (0.0, 0.25)
    mc = mask_components(torch.from_numpy(mask))
    assert mc.n(0) == 2 and mc.areas(0).tolist() == [100, 1] and corloc(mc.largest_boxes()) == (1.0, 1.0)
