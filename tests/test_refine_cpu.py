"""Image-guided refinement of word maps (include/daam_refine.h) without a GPU: ``libdaam_refine.so`` builds beside the
other libraries and exports what its header declares and the binding names; the header is C99; no kernel has scratch; every argument
the header rules out is refused before any HIP call; the float64 reference has the properties the contract states and sharpens a
blob to an ellipse's outline; and the Python layer (``engine.refine_affinity`` / ``refine_maps``, ``ImageAffinity``,
``GlobalHeatMap.refine``, ``Segmentation.refine``) on a numpy stand-in of the library.  The kernels run in ``test_gpu_refine.py``."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import _components_domain as C
import _libcheck as LC
import _refine_domain as R
from oracle import fake_diffusers as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
N_KERNELS = 13                      # affinity for 1 and 3 channels, apply for 1 2 3 4 6 8 12 16 24 32 accumulators, the copy


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build(verbose=False)
    return build.REFINE_LIB


@pytest.fixture(scope='module')
def lib(built):
    from daam_amd import _native as nat
    return nat.load_refine()


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_library_builds_and_exports_its_header(built, lib):
    from daam_amd import _native as nat, build
    assert os.path.exists(built) and os.path.basename(built) == 'libdaam_refine.so' and not build.refine_stale()
    assert build.REFINE_SOURCES == ['daam_refine.hip']
    exported = LC.exported(built)
    assert exported == LC.declared('daam_refine.h') == sorted(nat.REFINE_EXPORTS) and len(exported) == 6
    assert lib.daam_refine_abi_version() == 1 == nat.REFINE_ABI_VERSION
    assert len(lib.daam_refine_affinity.argtypes) == 9 and len(lib.daam_refine_apply.argtypes) == 15
    assert nat.REFINE_LIB_PATH == built or os.environ.get('DAAM_REFINE_LIB')
    names = list(build.kernel_shas(built))
    assert len(names) == N_KERNELS and sum('refine_apply_kernel' in n for n in names) == 10
    assert sum('refine_affinity_kernel' in n for n in names) == 2 and sum('refine_copy_kernel' in n for n in names) == 1


def test_refine_header_is_c99(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "daam_refine.h"\nint main(void) { return DAAM_REFINE_ABI_VERSION == 1 && sizeof(&daam_refine_apply) ? 0 : 1; }\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o',
                    str(tmp_path / 'use.o')], check=True)


def test_no_kernel_has_scratch_or_lds(built):
    """Private segment size 0, group segment size 0 and the private-segment enable bit clear in every kernel descriptor."""
    from daam_amd import build
    kds = LC.kernel_descriptors(built)
    names = list(build.kernel_shas(built))
    assert len(names) == N_KERNELS and all(k in kds for k in names)
    for k in names:
        group, private = struct.unpack_from('<II', kds[k], 0)
        _, rsrc2 = struct.unpack_from('<II', kds[k], 48)
        assert private == 0 and group == 0 and not (rsrc2 & 1), (k, group, private)


# ---- argument checks: all of them before any HIP call, so they run here ---------------------------------------------------------------
def _dil(values):
    return None if values is None else (ctypes.c_int32 * len(values))(*values)


def _affinity(lib, **over):
    a = dict(image=0x1000, h=37, w=53, channels=3, dilations=(1, 2, 4), n_dil=None, scale=0.1, weights=0x10000, stream=None)
    a.update(over)
    n_dil = len(a['dilations']) if a['n_dil'] is None else a['n_dil']
    rc = lib.daam_refine_affinity(a['image'], a['h'], a['w'], a['channels'], _dil(a['dilations']), n_dil, a['scale'], a['weights'], a['stream'])
    return rc, lib.daam_refine_last_error().decode()


def _apply(lib, **over):
    """A call that is in range but for ``over``; pointers are small fake addresses (nothing is dereferenced)."""
    a = dict(weights=0x100000, dilations=(1, 2, 4), n_dil=None, maps=0x1000000, n_maps=3, h=37, w=53, iterations=10, threshold=0.4,
             refined=0x2000000, masks=0x3000000, labels=0x4000000, workspace=0x5000000, workspace_bytes=None, stream=None)
    a.update(over)
    n_dil = len(a['dilations']) if a['n_dil'] is None else a['n_dil']
    if a['workspace_bytes'] is None:
        a['workspace_bytes'] = lib.daam_refine_workspace(a['n_maps'], a['h'], a['w']) or 1 << 20
    rc = lib.daam_refine_apply(a['weights'], _dil(a['dilations']), n_dil, a['maps'], a['n_maps'], a['h'], a['w'], a['iterations'],
                               a['threshold'], a['refined'], a['masks'], a['labels'], a['workspace'], a['workspace_bytes'], a['stream'])
    return rc, lib.daam_refine_last_error().decode()


BAD_GEOMETRY = {
    'no dilations': dict(dilations=(), n_dil=0), 'seven dilations': dict(dilations=(1, 2, 3, 4, 5, 6, 7)), 'dilation 0': dict(dilations=(0, 1)),
    'dilation 65': dict(dilations=(1, 65)), 'equal dilations': dict(dilations=(1, 2, 2)), 'falling dilations': dict(dilations=(4, 2)),
    'NULL dilations': dict(dilations=None, n_dil=2), 'h 0': dict(h=0), 'w 0': dict(w=0), '2^31 weights': dict(h=1 << 14, w=1 << 14, dilations=(1,)),
    '2^31 weights at six dilations': dict(h=6689, w=6689, dilations=(1, 2, 4, 8, 12, 24)),
}
BAD_AFFINITY = dict(BAD_GEOMETRY, **{
    '2 channels': dict(channels=2), '4 channels': dict(channels=4), 'scale 0': dict(scale=0.0), 'scale -1': dict(scale=-1.0),
    'scale inf': dict(scale=math.inf), 'scale nan': dict(scale=math.nan), 'NULL image': dict(image=None), 'NULL weights': dict(weights=None),
})
BAD_APPLY = dict(BAD_GEOMETRY, **{
    'no maps': dict(n_maps=0), '33 maps': dict(n_maps=33), 'iterations -1': dict(iterations=-1), 'iterations 65': dict(iterations=65),
    'threshold nan': dict(threshold=math.nan), 'threshold inf': dict(threshold=math.inf), 'NULL weights': dict(weights=None),
    'NULL maps': dict(maps=None), 'NULL refined': dict(refined=None), 'NULL workspace': dict(workspace=None),
    'small workspace': dict(workspace_bytes=4 * 3 * 37 * 53 - 4), 'refined is maps': dict(refined=0x1000000),
    'refined inside maps': dict(refined=0x1000000 + 4 * 3 * 37 * 53 - 4), 'refined is the workspace': dict(refined=0x5000000),
    'refined ends in the workspace': dict(refined=0x5000000 - 4 * 3 * 37 * 53 + 4),
    'refined inside a larger workspace': dict(refined=0x5000000 + (1 << 20), workspace_bytes=1 << 21),
})


@pytest.mark.parametrize('what', sorted(BAD_AFFINITY))
def test_affinity_out_of_range_is_refused_before_any_hip_call(lib, what):
    rc, msg = _affinity(lib, **BAD_AFFINITY[what])
    assert rc == E_INVALID and msg, (what, rc, msg)


@pytest.mark.parametrize('what', sorted(BAD_APPLY))
def test_apply_out_of_range_is_refused_before_any_hip_call(lib, what):
    rc, msg = _apply(lib, **BAD_APPLY[what])
    assert rc == E_INVALID and msg, (what, rc, msg)


def test_size_functions_agree_with_the_stand_in(lib):
    fake = R.FakeRefineLib()
    for h, w, n_dil in ((1, 1, 1), (37, 53, 3), (1024, 1024, 6), (5, 7, 6), (6688, 6688, 6), (1 << 14, (1 << 14) - 1, 1)):
        assert lib.daam_refine_weights_bytes(h, w, n_dil) == fake.daam_refine_weights_bytes(h, w, n_dil) == 32 * n_dil * h * w
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (4, 4, 7), (1 << 14, 1 << 14, 1), (6689, 6689, 6), (-1, 4, 1)):
        assert lib.daam_refine_weights_bytes(*bad) == 0 == fake.daam_refine_weights_bytes(*bad), bad
    for n, h, w in ((1, 1, 1), (3, 37, 53), (32, 1024, 1024), (1, 5, 7), (31, 3, 3)):
        got = lib.daam_refine_workspace(n, h, w)
        assert got == fake.daam_refine_workspace(n, h, w) == (4 * n * h * w + 7) // 8 * 8 and got % 8 == 0
    for bad in ((0, 4, 4), (33, 4, 4), (1, 0, 4), (1, 4, 0), (1, 1 << 14, 1 << 14)):
        assert lib.daam_refine_workspace(*bad) == 0 == fake.daam_refine_workspace(*bad), bad


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_a_flat_image_gives_one_over_k_everywhere():
    for c in (1, 3):
        assert set(R.reference_weights(R.image('flat', 5, 7, c), (1, 2)).ravel().tolist()) == {0.0625}
        w = R.reference_weights(R.image('flat', 9, 11, c))
        assert w.shape == (48, 9, 11) and set(w.ravel().tolist()) == {1 / 48}
        assert np.array_equal(R.emulate_weights(R.image('flat', 9, 11, c), (1, 2)), np.full((16, 9, 11), 0.0625, np.float32))


@pytest.mark.parametrize('kind', R.IMAGE_KINDS)
def test_weights_sum_to_one_and_outputs_stay_in_range(kind):
    for c, dil in ((1, (1,)), (3, (1, 2)), (3, R.DILATIONS)):
        img = R.image(kind, 13, 17, c, seed=3)
        w = R.reference_weights(img, dil)
        assert w.shape == (8 * len(dil), 13, 17) and (w >= 0).all()
        sums = np.array([math.fsum(w[:, y, x]) for y in range(13) for x in range(17)])
        assert np.abs(sums - 1).max() <= 2.0 ** -50
        m = R.maps(3, 13, 17, seed=1) * 3 - 1
        assert np.array_equal(R.reference_apply(w, dil, m, 0), m.astype(np.float64))              # T = 0 is the identity
        for t in (1, 4):
            out = R.reference_apply(w, dil, m, t)
            assert out.min() >= m.min() - 1e-12 and out.max() <= m.max() + 1e-12
            assert np.abs(R.emulate_apply(w.astype(np.float32), dil, m, t) - R.reference_apply(w.astype(np.float32), dil, m, t)).max() \
                <= R.apply_bound(w.astype(np.float32), m, t)


def test_neighbour_order_and_a_dilation_larger_than_the_image():
    qy, qx = R.neighbours(9, 11, (1, 3))
    assert [(int(qy[k, 4, 5]) - 4, int(qx[k, 4, 5]) - 5) for k in range(16)] == list(R.OFFSETS) + [(3 * dy, 3 * dx) for dy, dx in R.OFFSETS]
    qy, qx = R.neighbours(5, 7, (24,))
    for y in range(5):
        for x in range(7):                   # every coordinate that moves clamps to a border; one that does not move stays
            assert [(int(qy[k, y, x]), int(qx[k, y, x])) for k in range(8)] == \
                [((0, y, 4)[dy + 1] if dy else y, (0, x, 6)[dx + 1] if dx else x) for dy, dx in R.OFFSETS]
    img = R.image('random', 5, 7, 3, seed=5)
    w = R.reference_weights(img, (24,))
    m = R.maps(1, 5, 7)
    out = R.reference_apply(w, (24,), m, 1)[0]
    want = sum(w[k] * m[0][qy[k], qx[k]] for k in range(8))
    assert np.allclose(out, want, rtol=0, atol=1e-15)


def test_the_single_pixel_image_and_the_bounds_on_the_emulation():
    """One differing pixel: around it the neighbour that is the outlier gets (almost) no weight, elsewhere the weights are 1 / K; the
    f32 emulation stays inside bound (a), and far below it where the logits are zero."""
    img = R.image('pixel', 12, 15, 3)
    w = R.reference_weights(img, (1, 2))
    assert w[7, 5, 4] < 1e-15 and abs(w[0, 5, 4] - 1 / 15) < 1e-12          # (5, 4) sees the pixel (6, 5) as its neighbour (1, 1) at d = 1
    assert np.allclose(w[:, 0, 12], 0.0625, rtol=0, atol=0)
    for kind in R.IMAGE_KINDS:
        for c in (1, 3):
            im = R.image(kind, 21, 37, c, seed=2)
            err = np.abs(R.emulate_weights(im).astype(np.float64) - R.reference_weights(im))
            assert (err <= R.weights_bound(im)).all(), (kind, c, float((err / R.weights_bound(im)).max()))


def test_refinement_pulls_a_blob_onto_the_ellipse():
    """The reference itself: a Gaussian blob shifted off a noisy ellipse has IoU < 0.6 with it at 0.4 and >= 0.95 after ten
    iterations, rising on the way."""
    img, truth, plane = R.ellipse_case()
    soft = R.ellipse_soft(plane)
    w = R.reference_weights(img)
    got = [R.iou(R.reference_apply(w, R.DILATIONS, soft[None], t)[0] > 0.4, truth) for t in (0, 1, 2, 10)]
    assert got[0] < 0.6 and got[0] < got[1] < got[2] < got[3] and got[3] >= 0.95, got
    emu = R.emulate_apply(R.emulate_weights(img), R.DILATIONS, soft[None], 10)
    assert R.iou(emu[0] > 0.4, truth) >= 0.95
    masks, labels = R.outputs(emu, 0.4)
    assert np.array_equal(masks[0] != 0, emu[0] > np.float32(0.4)) and set(np.unique(labels)) == {0, 255}
    assert np.array_equal(labels == 0, masks[0] != 0)


def test_the_label_rule_takes_the_lowest_index_on_a_tie():
    r = np.array([[[0.5, 0.2]], [[0.5, 0.7]], [[0.1, 0.7]]], np.float32)
    masks, labels = R.outputs(r, 0.4)
    assert labels.tolist() == [[0, 1]] and masks[:, 0, 0].tolist() == [1, 1, 0]
    assert R.outputs(r, 0.7)[1].tolist() == [[255, 255]]                    # > is strict


# ---- the Python layer on the numpy stand-in --------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    return R.install(monkeypatch.setattr)


class _Image:
    def __init__(self, width, height):
        self.size = (width, height)             # PIL order


class _Pil(_Image):
    """As much of a PIL image as ``engine.refine_affinity`` touches."""

    def __init__(self, pixels, mode):
        super().__init__(pixels.shape[1], pixels.shape[0])
        self.pixels, self.mode = pixels, mode

    def convert(self, mode):
        assert mode == 'RGB'
        return _Pil(np.ascontiguousarray(self.pixels[:, :, :3]), 'RGB')

    def __array__(self, dtype=None, copy=None):
        return self.pixels


def test_refine_affinity_takes_every_form_of_image(fake):
    E, lib = fake
    rgb = R.image('edge', 12, 15, 3, seed=1)
    want = R.emulate_weights(rgb, (1, 2), 0.25)
    for form in (rgb, torch.from_numpy(rgb), _Pil(rgb, 'RGB'), _Pil(np.concatenate([rgb, rgb[:, :, :1]], axis=2), 'RGBA')):
        got = E.refine_affinity(form, (1, 2), scale=0.25)
        assert got.dtype == torch.float32 and got.shape == (16, 12, 15) and np.array_equal(got.numpy(), want)
        assert lib.calls[-1] == ('affinity', 12, 15, 3, (1, 2), 0.25)
    grey = rgb[:, :, 0].copy()
    for form in (grey, grey[:, :, None], torch.from_numpy(grey), _Pil(grey, 'L')):
        got = E.refine_affinity(form, (1, 2))
        assert np.array_equal(got.numpy(), R.emulate_weights(grey, (1, 2))) and lib.calls[-1][:5] == ('affinity', 12, 15, 1, (1, 2))
    assert E.refine_affinity(rgb).shape == (48, 12, 15) and lib.calls[-1][4] == R.DILATIONS
    with pytest.raises(RuntimeError):
        E.refine_affinity(rgb.astype(np.float32))
    for bad in (rgb[:, :, :2], rgb[None], rgb[0, :, 0]):
        with pytest.raises(ValueError):
            E.refine_affinity(bad)
    for bad in (dict(dilations=()), dict(dilations=(2, 1)), dict(dilations=(1, 65)), dict(dilations=range(1, 8)), dict(scale=0), dict(scale=math.nan)):
        with pytest.raises(ValueError):
            E.refine_affinity(rgb, **bad)


@pytest.mark.parametrize('n', [1, 32, 33, 65])
def test_refine_maps_runs_in_blocks_of_32(fake, n):
    E, lib = fake
    img = R.image('edge', 9, 13, 3)
    w = E.refine_affinity(img, (1, 3))
    m = np.tile(R.maps(5, 9, 13), (13, 1, 1))[:n]
    refined, masks, labels = E.refine_maps(w, (1, 3), torch.from_numpy(m), iterations=3, threshold=0.5, labels=n <= 32)
    want = R.emulate_apply(w.numpy(), (1, 3), m, 3)
    blocks = [32] * (n // 32) + ([n % 32] if n % 32 else [])
    assert [c[1] for c in lib.calls[1:]] == blocks and all(c[0] == 'apply' and c[2:] == (9, 13, (1, 3), 3, 0.5, True, n <= 32) for c in lib.calls[1:])
    assert refined.dtype == torch.float32 and refined.shape == (n, 9, 13) and np.array_equal(refined.numpy(), want)
    assert masks.dtype == torch.uint8 and np.array_equal(masks.numpy(), R.outputs(want, 0.5)[0])
    if n <= 32:
        assert labels.dtype == torch.uint8 and np.array_equal(labels.numpy(), R.outputs(want, 0.5)[1])
    else:
        assert labels is None
        with pytest.raises(ValueError):
            E.refine_maps(w, (1, 3), torch.from_numpy(m))
    plain = E.refine_maps(w, (1, 3), torch.from_numpy(m), iterations=0, masks=False, labels=False)
    assert plain[1] is None and plain[2] is None and np.array_equal(plain[0].numpy(), m) and lib.calls[-1][5:] == (0, float(np.float32(0.4)), False, False)


def test_refine_maps_refuses_what_does_not_fit(fake):
    E, _ = fake
    w = E.refine_affinity(R.image('edge', 9, 13, 3), (1, 3))
    m = torch.from_numpy(R.maps(2, 9, 13))
    for bad in (dict(dilations=(1,)), dict(dilations=(1, 2, 3)), dict(iterations=65), dict(iterations=-1), dict(threshold=math.inf)):
        kw = dict(dict(dilations=(1, 3)), **bad)
        with pytest.raises(ValueError):
            E.refine_maps(w, kw.pop('dilations'), m, **kw)
    with pytest.raises(ValueError, match='9 x 13.*9 x 12'):
        E.refine_maps(w, (1, 3), m[:, :, :12].contiguous())
    with pytest.raises(RuntimeError):
        E.refine_maps(w.double(), (1, 3), m)


PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


def _ghm(h=9, w=14):
    from daam_amd import GlobalHeatMap
    maps = torch.from_numpy(np.abs(np.random.default_rng(2).standard_normal((13, h, w))).astype(np.float32))
    return GlobalHeatMap(fd.FakeTokenizer(), PROMPT, maps)


def test_global_heat_map_refine_and_segmentation_refine_agree(fake, monkeypatch):
    from daam_amd import ImageAffinity, Segmentation, image_affinity
    E, lib = fake
    monkeypatch.setattr(E, 'word_masks', C.fake_word_masks([]))
    ghm = _ghm()
    img = R.image('edge', 45, 70, 3, seed=4)
    words = ['monkey', 'bicycle', ('photo', None)]
    seg = ghm.refine(words, img, threshold=0.5, iterations=2, dilations=(1, 2, 4), scale=0.2)
    assert [c[0] for c in lib.calls] == ['affinity', 'apply'] and lib.calls[0][1:] == (45, 70, 3, (1, 2, 4), float(np.float32(0.2)))
    assert lib.calls[1][1:] == (3, 45, 70, (1, 2, 4), 2, 0.5, True, True)
    assert isinstance(seg, Segmentation) and seg.words == ['monkey', 'bicycle', 'photo'] and len(seg.word_heat_maps) == 3
    soft = np.stack([R.D.emulate_expand(m.heatmap.numpy(), 45, 70) for m in seg.word_heat_maps])
    want = R.emulate_apply(R.emulate_weights(img, (1, 2, 4), 0.2), (1, 2, 4), soft, 2)
    assert seg.refined.dtype == torch.float32 and np.array_equal(seg.refined.numpy(), want)
    assert np.array_equal(seg.masks.numpy(), R.outputs(want, 0.5)[0]) and np.array_equal(seg.labels.numpy(), R.outputs(want, 0.5)[1])
    plain = ghm.segment(words, _Image(70, 45), threshold=0.5)                     # segment's size rule: rectangular maps -> [height, width]
    assert plain.masks.shape == seg.masks.shape and plain.refined is None
    again = plain.refine(img, threshold=0.5, iterations=2, dilations=(1, 2, 4), scale=0.2)
    for k in ('refined', 'masks', 'labels'):
        assert torch.equal(getattr(again, k), getattr(seg, k)), k
    assert again.words == seg.words

    aff = image_affinity(img, (1, 2, 4), 0.2)
    assert isinstance(aff, ImageAffinity) and aff.size == (45, 70) and aff.dilations == (1, 2, 4) and aff.scale == 0.2
    before = len(lib.calls)
    reuse = ghm.refine(words, _Image(70, 45), threshold=0.5, iterations=2, affinity=aff)        # the image's size is all that is read
    other = ghm.refine(['monkey'], img, threshold=0.3, iterations=1, affinity=aff, labels=False, absolute=True)
    assert [c[0] for c in lib.calls[before:]] == ['apply', 'apply'] and torch.equal(reuse.refined, seg.refined)
    assert other.labels is None and other.masks.shape == (1, 45, 70) and lib.calls[-1][5:] == (1, float(np.float32(0.3)), True, False)
    host = seg.cpu()
    assert torch.equal(host.refined, seg.refined) and torch.equal(host.masks, seg.masks) and plain.cpu().refined is None
    with pytest.raises(ValueError, match='45 x 70.*70 x 45'):
        ghm.refine(words, _Image(45, 70), affinity=aff)
    with pytest.raises(ValueError):
        ghm.refine([], img)
    with pytest.raises(TypeError):
        ghm.refine(words, img, affinity=aff.weights)
    with pytest.raises(ValueError):
        Segmentation(['w'] * 33, seg.word_heat_maps * 11, seg.masks, None).refine(img)
    many = Segmentation(['w'] * 33, seg.word_heat_maps * 11, seg.masks, None).refine(img, iterations=1, labels=False, affinity=aff)
    assert many.refined.shape == (33, 45, 70) and [c[1] for c in lib.calls[-2:]] == [32, 1]


def test_segmentation_still_takes_four_positional_arguments():
    from daam_amd import Segmentation
    masks = torch.zeros(1, 4, 4, dtype=torch.uint8)
    seg = Segmentation(['a'], [], masks, None)
    assert seg.refined is None and seg.labels is None and seg.masks is masks
    assert Segmentation(['a'], [], masks, None, torch.ones(1, 4, 4)).refined.shape == (1, 4, 4)


def test_the_ellipse_through_the_python_layer(fake):
    """``GlobalHeatMap.refine`` on the prompt's word whose plane is the shifted Gaussian: IoU with the ellipse < 0.6 from ``segment``,
    >= 0.95 refined."""
    from daam_amd import GlobalHeatMap
    img, truth, plane = R.ellipse_case()
    maps = torch.zeros(13, *R.ELLIPSE_PLANE)
    ghm = GlobalHeatMap(fd.FakeTokenizer(), PROMPT, maps)
    from daam_amd.utils import compute_token_merge_indices
    for i in compute_token_merge_indices(ghm.tokenizer, PROMPT, 'bicycle', None)[0]:
        maps[i] = torch.from_numpy(plane)
    seg = ghm.refine(['bicycle'], img)
    before = R.D.emulate_expand(plane, *R.ELLIPSE) > np.float32(0.4)
    assert R.iou(before, truth) < 0.6 and R.iou(seg.masks[0].numpy(), truth) >= 0.95
    assert np.array_equal(seg.labels.numpy() == 0, seg.masks[0].numpy() != 0)
