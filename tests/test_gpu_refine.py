"""``daam_refine_affinity`` / ``daam_refine_apply`` (include/daam_refine.h) on the device, through ctypes on guarded
buffers and through the Python layer, held to the float64 reference of ``_refine_domain`` inside the two bounds derived there:
(a) every weight, absolutely; (b) the refined maps against float64 fed the device's own weights; and both combined against the pure
float64 path.  Masks and labels are held EXACTLY to the rules evaluated on the device's own refined values.

A workgroup's tile is 4 rows x 64 columns (one wave per row).  The shapes: 1 x 1; 5 x 7 (every neighbour of the larger dilations
clamps); 37 x 70 (ten tile rows, the last partial; a column seam and a 6-column partial tile); 64 x 64 (whole tiles only); 33 x 130
(three tile columns, the last 2 wide; a 1-row partial tile); 11 x 150 (three tile rows by three tile columns, partial on both
edges).  Figures of every case are printed before they are asserted (``pytest -s``)."""
import numpy as np
import pytest
import torch

import _refine_domain as R
from oracle import fake_diffusers as fd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64                       # guard bytes on either side of a buffer
THRESHOLD = 0.4


def _guarded(n_bytes, fill, offset=0):
    """A uint8 device buffer of ``n_bytes`` at ``offset`` bytes past 16-byte alignment, between two guards of 0xA5, filled with ``fill``."""
    raw = torch.full((GUARD + 16 + n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(raw.data_ptr() + GUARD) % 16) + offset
    raw[start:start + n_bytes] = fill
    return raw, start


def _put(buf, array):
    raw, start = buf
    flat = torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).reshape(-1)).to(DEV)
    raw[start:start + flat.numel()] = flat


def _get(buf, n_bytes, dtype, shape):
    raw, start = buf
    return raw[start:start + n_bytes].cpu().numpy().view(dtype).reshape(shape).copy()


def _intact(buf, n_bytes):
    raw, start = buf
    return bool((raw[:start] == 0xA5).all()) and bool((raw[start + n_bytes:] == 0xA5).all())


def _dil(dilations):
    import ctypes
    return (ctypes.c_int32 * len(dilations))(*dilations)


def affinity_raw(image, dilations, scale=0.1, image_offset=3):
    """One ``daam_refine_affinity`` call on guarded buffers (the image at an odd byte offset, the weights pre-filled with 0xFF):
    f32 [K, h, w], after checking the guards and that the image is unchanged."""
    from daam_amd import _native as nat
    lib = nat.load_refine()
    px = image[:, :, None] if image.ndim == 2 else image
    h, w, c = px.shape
    n_w = lib.daam_refine_weights_bytes(h, w, len(dilations))
    assert n_w == 32 * len(dilations) * h * w
    img, wts = _guarded(h * w * c, 0, image_offset), _guarded(n_w, 0xFF, 4)
    _put(img, px)
    before = img[0].clone()
    nat.check_refine(lib.daam_refine_affinity(img[0].data_ptr() + img[1], h, w, c, _dil(dilations), len(dilations), scale,
                                              wts[0].data_ptr() + wts[1], torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _intact(img, h * w * c) and _intact(wts, n_w), 'guard bytes changed'
    assert torch.equal(img[0], before), 'the image changed'
    return _get(wts, n_w, np.float32, (8 * len(dilations), h, w))


def apply_raw(weights, dilations, maps, iterations, threshold=THRESHOLD, masks=True, labels=True):
    """One ``daam_refine_apply`` call on guarded buffers: outputs pre-filled with 0xFF, a workspace of exactly the bytes asked for
    (pre-filled with 0x5A), masks and labels at odd byte offsets.  Returns ``(refined, masks or None, labels or None)`` after checking
    every guard and that weights and maps are unchanged."""
    from daam_amd import _native as nat
    lib = nat.load_refine()
    n, h, w = maps.shape
    need = lib.daam_refine_workspace(n, h, w)
    assert need >= 4 * n * h * w and need % 8 == 0
    sizes = dict(weights=weights.nbytes, maps=maps.nbytes, refined=maps.nbytes, ws=need, masks=n * h * w if masks else 0, labels=h * w if labels else 0)
    offsets = dict(weights=4, maps=8, refined=12, ws=8, masks=1, labels=7)
    bufs = {k: _guarded(v, 0x5A if k == 'ws' else 0xFF, offsets[k]) for k, v in sizes.items() if v}
    _put(bufs['weights'], weights)
    _put(bufs['maps'], maps)
    before = {k: bufs[k][0].clone() for k in ('weights', 'maps')}
    ptr = lambda k: bufs[k][0].data_ptr() + bufs[k][1] if k in bufs else None
    nat.check_refine(lib.daam_refine_apply(ptr('weights'), _dil(dilations), len(dilations), ptr('maps'), n, h, w, iterations, threshold,
                                           ptr('refined'), ptr('masks'), ptr('labels'), ptr('ws'), need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for k in bufs:
        assert _intact(bufs[k], sizes[k]), f'guard bytes around {k} changed'
    assert all(torch.equal(bufs[k][0], before[k]) for k in before), 'weights or maps changed'
    return (_get(bufs['refined'], maps.nbytes, np.float32, (n, h, w)), _get(bufs['masks'], n * h * w, np.uint8, (n, h, w)) if masks else None,
            _get(bufs['labels'], h * w, np.uint8, (h, w)) if labels else None)


# (h, w, channels, dilations, maps, iterations, image)
CASES = [
    (1, 1, 3, (1,), 1, 1, 'flat'), (1, 1, 1, R.DILATIONS, 3, 10, 'random'), (5, 7, 3, R.DILATIONS, 3, 2, 'random'), (5, 7, 1, (1, 2), 1, 10, 'pixel'),
    (37, 70, 3, R.DILATIONS, 3, 10, 'edge'), (37, 70, 1, (1, 2), 1, 1, 'pixel'), (64, 64, 3, (1,), 32, 2, 'random'),
    (64, 64, 1, R.DILATIONS, 1, 0, 'edge'), (33, 130, 3, R.DILATIONS, 32, 10, 'edge'), (33, 130, 3, (1, 2), 3, 1, 'flat'),
    (11, 150, 1, R.DILATIONS, 3, 10, 'random'), (11, 150, 3, (1,), 32, 0, 'pixel'), (11, 150, 3, (1, 2), 32, 10, 'edge'),
    (33, 130, 1, R.DILATIONS, 3, 2, 'pixel'),
]


@pytest.mark.parametrize('h,w,c,dil,n,t,kind', CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_weights_and_refined_maps_are_within_their_bounds(h, w, c, dil, n, t, kind):
    img = R.image(kind, h, w, c, seed=h + w)
    maps = R.maps(n, h, w, seed=n)
    weights = affinity_raw(img, dil)
    assert np.array_equal(weights, affinity_raw(img, dil, image_offset=0)), 'a second run of the weights'
    ref_w = R.reference_weights(img, dil)
    bound_a = R.weights_bound(img, dil)
    err_a = np.abs(weights.astype(np.float64) - ref_w)
    emu_a = np.abs(R.emulate_weights(img, dil).astype(np.float64) - ref_w)
    print(f'\n{h}x{w} C={c} K={8 * len(dil)} N={n} T={t} {kind}: weights emulation {emu_a.max():.3e} device {err_a.max():.3e} '
          f'bound {bound_a.max():.3e} worst device/bound {(err_a / bound_a).max():.3f}')
    assert (err_a <= bound_a).all(), f'weights: {(err_a / bound_a).max():.3f} of the bound'
    if kind == 'flat':
        assert (weights == np.float32(1.0 / (8 * len(dil)))).all()
    assert weights.min() >= 0 and abs(R.weight_sum(weights) - 1) <= (8 * len(dil) + 2) * R.U

    refined, masks, labels = apply_raw(weights, dil, maps, t)
    again = apply_raw(weights, dil, maps, t)
    assert all(np.array_equal(a, b) for a, b in zip((refined, masks, labels), again)), 'a second run'
    fed = R.reference_apply(weights, dil, maps, t)
    pure = R.reference_apply(ref_w, dil, maps, t)
    bound_b, bound_ab = R.apply_bound(weights, maps, t), R.combined_bound(img, dil, 0.1, weights, maps, t)
    err_b, err_ab = np.abs(refined - fed).max(), np.abs(refined - pure).max()
    emu_b = np.abs(R.emulate_apply(weights, dil, maps, t) - fed).max()
    print(f'    refined emulation {emu_b:.3e} device {err_b:.3e} bound {bound_b:.3e}; end to end device {err_ab:.3e} bound {bound_ab:.3e}')
    if t == 0:
        assert np.array_equal(refined.view(np.uint32), maps.view(np.uint32)), 'iterations = 0 returns the input bits'
    assert err_b <= bound_b and err_ab <= bound_ab
    # a convex combination up to rounding: the weights sum to 1 within K u and a chain adds g, T times over: twice bound (b)
    assert refined.min() >= maps.min() - 2 * bound_b and refined.max() <= maps.max() + 2 * bound_b
    want_masks, want_labels = R.outputs(refined, THRESHOLD)
    assert np.array_equal(masks, want_masks) and np.array_equal(labels, want_labels)
    none = apply_raw(weights, dil, maps, t, masks=False, labels=False)
    assert none[1] is None and none[2] is None and np.array_equal(none[0], refined)


def test_the_label_rule_on_ties_and_thresholds_of_any_sign():
    """Maps 0 and 1 are equal, so every pixel they own is a tie: the label is 0.  A threshold above every value gives 255 and empty
    masks, one below every value gives full masks."""
    img, maps = R.image('edge', 11, 150, 3), R.maps(3, 11, 150)
    weights = affinity_raw(img, (1, 2))
    refined, masks, labels = apply_raw(weights, (1, 2), maps, 2)
    assert np.array_equal(refined[0], refined[1]) and not (labels == 1).any() and (labels == 0).any() and (labels == 2).any()
    for thr, full in ((2.0, 0), (-1.0, 1)):
        r2, m2, l2 = apply_raw(weights, (1, 2), maps, 2, threshold=thr)
        assert np.array_equal(r2, refined) and (m2 == full).all() and ((l2 == 255).all() if not full else (l2 < 3).all())


# ---- Python ----------------------------------------------------------------------------------------------------------------------------
PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


class _Image:
    def __init__(self, width, height):
        self.size = (width, height)             # PIL order


def _ellipse_ghm():
    from daam_amd import GlobalHeatMap
    from daam_amd.utils import compute_token_merge_indices
    img, truth, plane = R.ellipse_case()
    maps = 0.1 * np.abs(np.random.default_rng(5).standard_normal((13,) + R.ELLIPSE_PLANE)).astype(np.float32)
    tok = fd.FakeTokenizer()
    for i in compute_token_merge_indices(tok, PROMPT, 'bicycle', None)[0]:
        maps[i] = plane
    return GlobalHeatMap(tok, PROMPT, torch.from_numpy(maps).to(DEV)), img, truth, plane


def test_the_ellipse_through_global_heat_map_refine():
    """The IoU gain of the CPU test on the device: < 0.6 from ``segment``, >= 0.95 after ten iterations; ``Segmentation.refine`` and a
    reused ``ImageAffinity`` give the same bits; the refined maps are the reference's."""
    from daam_amd import Segmentation, image_affinity
    ghm, img, truth, plane = _ellipse_ghm()
    words = ['bicycle', 'monkey', ('photo', None)]
    plain = ghm.segment(words, _Image(70, 45), threshold=THRESHOLD)
    seg = ghm.refine(words, img, threshold=THRESHOLD)
    assert isinstance(seg, Segmentation) and seg.masks.is_cuda and seg.refined.is_cuda and seg.refined.dtype == torch.float32
    assert seg.masks.shape == plain.masks.shape == (3, 45, 70) and seg.labels.shape == (45, 70) and plain.refined is None
    before, after = R.iou(plain.masks[0].cpu().numpy(), truth), R.iou(seg.masks[0].cpu().numpy(), truth)
    print(f'\nellipse: IoU {before:.3f} -> {after:.3f}')
    assert before < 0.6 and after >= 0.95
    again = plain.refine(img, threshold=THRESHOLD)
    aff = image_affinity(torch.from_numpy(img), scale=0.1)
    reuse = ghm.refine(words, img, threshold=THRESHOLD, affinity=aff)
    for k in ('refined', 'masks', 'labels'):
        assert torch.equal(getattr(again, k), getattr(seg, k)) and torch.equal(getattr(reuse, k), getattr(seg, k)), k
    refined = seg.refined.cpu().numpy()
    want_masks, want_labels = R.outputs(refined, THRESHOLD)
    assert np.array_equal(seg.masks.cpu().numpy(), want_masks) and np.array_equal(seg.labels.cpu().numpy(), want_labels)
    from daam_amd import engine as E
    soft = torch.stack([E.expand_word_map(m.heatmap, 45, 70) for m in seg.word_heat_maps]).cpu().numpy()
    weights = aff.weights.cpu().numpy()
    assert np.abs(refined - R.reference_apply(weights, R.DILATIONS, soft, 10)).max() <= R.apply_bound(weights, soft, 10)
    assert (np.abs(weights - R.reference_weights(img)) <= R.weights_bound(img)).all()
    assert seg.iou(torch.from_numpy(truth)).shape == (3, 1) and seg.components().n(0) >= 1 and seg.clean(largest=True).masks.shape == (3, 45, 70)
    host = seg.cpu()
    assert not host.refined.is_cuda and np.array_equal(host.refined.numpy(), refined)
    with pytest.raises(ValueError, match='45 x 70.*30 x 70'):
        ghm.refine(words, np.zeros((30, 70, 3), np.uint8), affinity=aff)


def test_engine_refine_maps_in_blocks_and_its_refusals():
    from daam_amd import engine as E
    img = R.image('edge', 33, 130, 3, seed=9)
    maps = np.tile(R.maps(5, 33, 130, seed=2), (7, 1, 1))[:34]
    w = E.refine_affinity(img, (1, 2, 4), scale=0.2)
    assert w.is_cuda and w.shape == (24, 33, 130) and torch.equal(w, E.refine_affinity(torch.from_numpy(img).to(DEV), (1, 2, 4), scale=0.2))
    assert (np.abs(w.cpu().numpy() - R.reference_weights(img, (1, 2, 4), 0.2)) <= R.weights_bound(img, (1, 2, 4), 0.2)).all()
    dev_maps = torch.from_numpy(maps).to(DEV)
    refined, masks, labels = E.refine_maps(w, (1, 2, 4), dev_maps, iterations=3, threshold=0.5, labels=False)
    assert labels is None and refined.shape == (34, 33, 130) and masks.dtype == torch.uint8
    got = refined.cpu().numpy()
    assert np.abs(got - R.reference_apply(w.cpu().numpy(), (1, 2, 4), maps, 3)).max() <= R.apply_bound(w.cpu().numpy(), maps, 3)
    assert np.array_equal(masks.cpu().numpy(), R.outputs(got, 0.5)[0])
    first = E.refine_maps(w, (1, 2, 4), dev_maps[:32], iterations=3, threshold=0.5)
    assert torch.equal(first[0], refined[:32]) and np.array_equal(first[2].cpu().numpy(), R.outputs(got[:32], 0.5)[1])
    grey = E.refine_affinity(img[:, :, 0].copy(), (1,))
    assert (np.abs(grey.cpu().numpy() - R.reference_weights(img[:, :, 0], (1,))) <= R.weights_bound(img[:, :, 0], (1,))).all()
    with pytest.raises(ValueError):
        E.refine_maps(w, (1, 2, 4), dev_maps)                                  # a label map of 34 maps
    with pytest.raises(RuntimeError):
        E.refine_maps(w, (1, 2, 4), torch.from_numpy(maps))                    # maps on the host
    with pytest.raises(RuntimeError):
        E.refine_maps(w, (1, 2, 4), dev_maps.double())
    with pytest.raises(ValueError, match='33 x 130.*33 x 129'):
        E.refine_maps(w, (1, 2, 4), dev_maps[:, :, :129].contiguous())
