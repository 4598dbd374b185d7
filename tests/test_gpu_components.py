"""``daam_mask_components`` (include/daam_components.h) on the device, through ctypes and through the Python layer:
every integer the call returns equals the numpy reference of ``_components_domain`` (union-find over row runs, held to
``scipy.ndimage`` and to a breadth-first search in ``test_components_cpu.py``), on both connectivities.  The shapes reach every seam
case of the kernels' 32 x 256 tile: 67 x 531 is three tile rows by three tile columns with partial tiles on both edges."""
import numpy as np
import pytest
import torch

import _components_domain as C
import _locate_domain as L
from oracle import fake_diffusers as fd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64                       # guard bytes on either side of a buffer
KEYS = ('labels', 'counts', 'comps', 'largest', 'kept')


def _guarded(n_bytes, fill, offset=0):
    """A uint8 device buffer of ``n_bytes`` at ``offset`` bytes past 16-byte alignment, between two guards of 0xA5, filled with ``fill``."""
    raw = torch.full((GUARD + 16 + n_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    start = GUARD + (-(raw.data_ptr() + GUARD) % 16) + offset
    raw[start:start + n_bytes] = fill
    return raw, start


def _guards_intact(raw, start, n_bytes):
    return bool((raw[:start] == 0xA5).all()) and bool((raw[start + n_bytes:] == 0xA5).all())


def components_raw(masks, connectivity=8, min_area=0, keep=0, max_comp=256, labels=True, mask_offset=0, ws_offset=0, on_device=False):
    """One ``daam_mask_components`` call through ctypes on guarded buffers: outputs pre-filled with 0xFF, a workspace of exactly the
    bytes asked for (pre-filled with 0x5A), the masks at ``mask_offset`` bytes past alignment.  Returns a dict of numpy arrays (device
    tensors with ``on_device``; None where the call has none) after checking every guard and that the masks are unchanged."""
    from daam_amd import _native as nat
    lib = nat.load_components()
    masks = np.ascontiguousarray(masks, np.uint8)
    n, h, w = masks.shape
    need = lib.daam_mask_components_workspace(n, h, w, max_comp)
    assert need > 0 and need % 8 == 0
    sizes = dict(ws=need, labels=4 * n * h * w if labels else 0, counts=8 * n, comps=24 * n * max_comp, largest=24 * n, kept=n * h * w if keep else 0)
    bufs = {k: _guarded(v, 0x5A if k == 'ws' else 0xFF, ws_offset if k == 'ws' else 0) for k, v in sizes.items() if v}
    sizes['masks'] = n * h * w
    bufs['masks'] = raw, start = _guarded(n * h * w, 0, mask_offset)
    raw[start:start + n * h * w] = torch.from_numpy(masks).to(DEV).reshape(-1)
    before = raw.clone()
    ptr = lambda k: bufs[k][0].data_ptr() + bufs[k][1] if k in bufs else None
    nat.check_components(lib.daam_mask_components(ptr('masks'), n, h, w, connectivity, min_area, keep, max_comp, ptr('labels'), ptr('counts'),
                                                  ptr('comps'), ptr('largest'), ptr('kept'), ptr('ws'), need,
                                                  torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for k, (raw, start) in bufs.items():
        assert _guards_intact(raw, start, sizes[k]), f'guard bytes around {k} changed'
    assert torch.equal(bufs['masks'][0], before), 'the mask bytes changed'

    def arr(k, dtype, shape):
        if k not in bufs:
            return None
        raw, start = bufs[k]
        flat = raw[start:start + sizes[k]]
        return flat.clone().view(dtype).reshape(shape) if on_device else flat.cpu().numpy().view(np.dtype(str(dtype).split('.')[-1])).reshape(shape)
    return dict(labels=arr('labels', torch.int32, (n, h, w)), counts=arr('counts', torch.int32, (n, 2)), comps=arr('comps', torch.int32, (n, max_comp, 6)),
                largest=arr('largest', torch.int32, (n, 6)), kept=arr('kept', torch.uint8, (n, h, w)))


def _same(got, want, what, labels=True):
    for k in KEYS:
        if want[k] is None or (k == 'labels' and not labels) or (k == 'comps' and want[k].shape[1] == 0):
            assert got[k] is None or got[k].size == 0, (what, k)
            continue
        bad = int((got[k] != want[k]).sum())
        assert bad == 0, f'{what}: {k} differs at {bad} of {want[k].size} integers'


def _check(masks, what, connectivity, **kw):
    ref_kw = {k: v for k, v in kw.items() if k in ('min_area', 'keep', 'max_comp')}
    got = components_raw(masks, connectivity, **kw)
    _same(got, C.reference(masks, connectivity, **ref_kw), what, kw.get('labels', True))
    return got


# ---- size, fill, alignment -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('connectivity', [4, 8])
def test_tiny_empty_and_full_planes(connectivity):
    for hw in ((1, 1), (1, 37), (37, 1), (52, 76), C.SEAMS):
        stack = np.stack([np.zeros(hw, np.uint8), np.full(hw, 128, np.uint8), C.noise(*hw, seed=5)])
        got = _check(stack, hw, connectivity, keep=2, max_comp=3)
        assert got['largest'][0].tolist() == C.sentinel(*hw) and not got['kept'][0].any() and (got['labels'][0] == -1).all()
        assert got['largest'][1].tolist() == [0, hw[0] * hw[1], 0, 0, hw[1] - 1, hw[0] - 1] and got['counts'][1].tolist() == [1, 1]
        assert got['kept'][1].all() and not got['labels'][1].any() and (got['comps'][0] == C.sentinel(*hw)).all()


@pytest.mark.parametrize('connectivity', [4, 8])
def test_every_seam_case_of_a_tile(connectivity):
    """The hand-made masks over 67 x 531 in ONE call of 32 masks (the 13 shapes, then noise of other seeds and fills), and some of
    them alone: a spiral and two combs (long parent chains, the same seam crossed many times), a U whose arms join only in the tile
    below (two local roots merge to the lower), a ring around a blob, pixels that touch only across a tile corner, equal areas."""
    names = sorted(C.SEAM_MASKS)
    stack = np.stack([C.SEAM_MASKS[n](*C.SEAMS) for n in names] + [C.noise(*C.SEAMS, seed=s, fill=0.3 + 0.02 * s) for s in range(32 - len(names))])
    want = C.reference(stack, connectivity, 6, 1, 64)
    full = components_raw(stack, connectivity, min_area=6, keep=1, max_comp=64)
    _same(full, want, 'the 32-mask call')
    again = components_raw(stack, connectivity, min_area=6, keep=1, max_comp=64)
    assert all(np.array_equal(full[k], again[k]) for k in KEYS), 'a second run'
    for name in ('spiral', 'comb', 'u', 'corners', 'ties', 'noise'):
        m = names.index(name)
        alone = components_raw(stack[m:m + 1], connectivity, min_area=6, keep=1, max_comp=64)
        assert all(np.array_equal(alone[k][0], full[k][m]) for k in KEYS), name
    u, ties, corners = (full[k] for k in ('largest', 'largest', 'counts'))
    assert u[names.index('u')].tolist()[:2] == [3 * 531 + 200, 36 + 38 + 191 - 2] and ties[names.index('ties')].tolist() == [532, 6, 1, 1, 3, 2]
    assert corners[names.index('corners'), 0] == (4 if connectivity == 4 else 2) and full['counts'][names.index('spiral')].tolist() == [1, 1]


def test_checkerboard_more_components_than_rows():
    board = C.checkerboard(52, 76)[None] * np.uint8(255)
    for max_comp in (4, 0):
        four = _check(board, ('checker', 4, max_comp), 4, max_comp=max_comp, min_area=2, keep=1)
        assert four['counts'].tolist() == [[52 * 76 // 2, 0]] and not four['kept'].any() and four['largest'][0].tolist() == [0, 1, 0, 0, 0, 0]
        eight = _check(board, ('checker', 8, max_comp), 8, max_comp=max_comp, keep=2)
        assert eight['counts'].tolist() == [[1, 1]] and eight['largest'][0].tolist() == [0, 52 * 76 // 2, 0, 0, 75, 51]
    assert four['comps'] is None and _check(board, 'four rows', 4, max_comp=4)['comps'][0, :, 0].tolist() == [0, 2, 4, 6]
    wide = _check(C.checkerboard(*C.SEAMS)[None], 'checker over seams', 4, max_comp=65536)        # every root listed: ranks across tile columns
    assert wide['counts'][0, 0] == (67 * 531 + 1) // 2 and wide['comps'][0, 300, 0] == 531 + 2 * (300 - 266) + 1


@pytest.mark.parametrize('connectivity', [4, 8])
def test_min_area_keep_and_no_labels(connectivity):
    stack = np.stack([C.blobs(52, 76, seed=s, n=4, speckle=0.03) for s in range(3)] + [C.equal_areas(*C.SEAMS)[:52, :76] * np.uint8(2)])
    areas = C.reference(stack, connectivity)['comps'][0, :, 1]
    area = int(np.sort(areas[areas > 0])[-2])                                     # the second largest area of the first mask
    for min_area in (area, area + 1):
        for keep in (1, 2):
            got = _check(stack, (min_area, keep), connectivity, min_area=min_area, keep=keep, max_comp=16)
            none = _check(stack, (min_area, keep, 'no labels'), connectivity, min_area=min_area, keep=keep, max_comp=16, labels=False)
            assert none['labels'] is None and all(np.array_equal(none[k], got[k]) for k in KEYS[1:])
        assert got['counts'][0, 1] == (2 if min_area == area else 1)
    assert _check(stack, 'keep 0', connectivity, min_area=3, keep=0)['kept'] is None


def test_mask_bytes_at_any_alignment():
    """Set bytes 1, 2, 128 and 255 count alike; the stack at odd byte offsets with odd plane sizes (52 x 77 = 4004, 67 x 531); a
    workspace 8 bytes past 16-byte alignment."""
    for hw in ((52, 77), C.SEAMS):
        stack = np.stack([C.blobs(*hw, seed=2, speckle=0.01), C.noise(*hw, seed=4), C.spiral(*hw) * np.uint8(128)])
        assert {1, 2, 128, 255} <= set(np.unique(stack))
        base = _check((stack != 0).astype(np.uint8), hw, 8, keep=2, max_comp=32)
        for offset in (1, 3, 7, 15):
            got = components_raw(stack, 8, keep=2, max_comp=32, mask_offset=offset)
            assert all(np.array_equal(got[k], base[k]) for k in KEYS), (hw, offset)
        got = components_raw(stack, 8, keep=2, max_comp=32, ws_offset=8)
        assert all(np.array_equal(got[k], base[k]) for k in KEYS)


def test_a_full_call_of_32_masks_at_1024():
    """Blobs and speckles at 1024 x 1024, four distinct masks eight times over: compared on the device."""
    distinct = np.stack([C.blobs(1024, 1024, seed=s) for s in range(4)])
    want = C.reference(distinct, 8, 50, 1, 256)
    got = components_raw(np.tile(distinct, (8, 1, 1)), 8, min_area=50, keep=1, max_comp=256, on_device=True)
    for k in KEYS:
        ref = torch.from_numpy(want[k]).to(DEV)
        for rep in range(8):
            assert torch.equal(got[k][4 * rep:4 * rep + 4], ref), (k, rep)
    assert want['counts'][:, 0].min() > 100 and (want['counts'][:, 1] < want['counts'][:, 0]).all()


# ---- Python -------------------------------------------------------------------------------------------------------------------------------
class _Image:
    def __init__(self, width, height):
        self.size = (width, height)             # PIL order


PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


def _ghm(h, w):
    from daam_amd import GlobalHeatMap
    rng = np.random.default_rng(17)
    yy, xx = np.mgrid[0:h, 0:w]
    maps = np.stack([np.exp(-((yy - rng.uniform(0, h)) ** 2 + (xx - rng.uniform(0, w)) ** 2) / (2 * (0.12 * h) ** 2)) +
                     0.6 * np.exp(-((yy - rng.uniform(0, h)) ** 2 + (xx - rng.uniform(0, w)) ** 2) / (2 * (0.06 * h) ** 2)) +
                     0.05 * np.abs(rng.standard_normal((h, w))) for _ in range(13)]).astype(np.float32)
    return GlobalHeatMap(fd.FakeTokenizer(), PROMPT, torch.from_numpy(maps).to(DEV))


def test_mask_components_and_clean_on_the_device():
    from daam_amd import Segmentation, mask_components
    stack = np.stack([C.blobs(67, 300, seed=s, n=4, speckle=0.01) for s in range(34)])           # two blocks of masks
    mc = mask_components(torch.from_numpy(stack).to(DEV), connectivity=4, min_area=9, keep='area', max_components=12)
    want = C.reference(stack, 4, 9, 1, 12)
    assert mc.labels.is_cuda and mc.labels.dtype == torch.int32 and mc.kept.dtype == torch.uint8
    host = mc.cpu()
    assert all(np.array_equal(getattr(host, k).numpy(), want[j]) for k, j in zip(('labels', 'counts', 'components', 'largest', 'kept'), KEYS))
    assert mc.n(33) == want['counts'][33, 0] and np.array_equal(mc.boxes(5).cpu().numpy(), want['comps'][5, :min(mc.n(5), 12), 2:])
    seg = Segmentation(['w%d' % i for i in range(34)], [], torch.from_numpy(stack).to(DEV), None)
    clean = seg.clean(largest=True)
    assert clean.masks.is_cuda and np.array_equal(clean.masks.cpu().numpy(), C.reference(stack, 8, 0, 2)['kept']) and clean.labels is None
    assert torch.equal(seg.components().largest_boxes(), torch.from_numpy(C.reference(stack, 8)['largest'][:, 2:]).to(DEV))
    assert torch.equal(clean.iou(seg.masks).diagonal() <= 1, torch.ones(34, dtype=torch.bool, device=DEV))


def test_localize_largest_component_equals_the_reference():
    from daam_amd import LocalizationEvaluator
    ghm = _ghm(16, 24)
    words, image = ['monkey', 'bicycle', ('photo', None)], _Image(300, 67)
    truth = torch.from_numpy(C.blobs(67, 300, seed=1, n=3, speckle=0)).to(DEV)
    thr = [0.3, 0.5, 0.75]
    plain = ghm.localize(words, image, thr, truth)
    loc = ghm.localize(words, image, thr, truth, component='largest')
    assert loc.boxes.is_cuda and loc.boxes.shape == (3, 3, 4) and loc.boxes.dtype == torch.int32 and loc.size == (67, 300)
    differs = 0
    for t, tau in enumerate(thr):
        masks = ghm.segment(words, image, threshold=tau, labels=False).masks.cpu().numpy()
        want = C.reference(masks, 8)['largest'][:, 2:]
        assert np.array_equal(loc.boxes[:, t].cpu().numpy(), want), tau
        assert np.array_equal(plain.boxes[:, t].cpu().numpy(), L.mask_boxes(masks))
        differs += int((want != L.mask_boxes(masks)).any())
    assert differs, 'two bumps per plane: at some threshold the whole-mask box is not the largest blob\'s'
    for k in ('peaks', 'peak_values', 'truth_boxes', 'hits'):
        assert torch.equal(getattr(loc, k), getattr(plain, k)), k
    assert len(LocalizationEvaluator().log(loc)) == 3 and loc.box_iou().shape == (3, 1, 3)


def test_a_speckle_stretches_the_whole_mask_box_only():
    from daam_amd import mask_boxes, mask_components
    mask = np.zeros((300, 600), np.uint8)
    mask[20:120, 200:330] = 255                                                   # crosses tile rows and a tile column
    mask[299, 0] = 1
    dev = torch.from_numpy(mask).to(DEV)
    assert mask_boxes(dev).tolist() == [[0, 20, 329, 299]]
    mc = mask_components(dev)
    assert mc.largest_boxes().tolist() == [[200, 20, 329, 119]] and mc.n() == 2 and mc.areas().tolist() == [13000, 1]
    assert mc.labels[0, 299, 0] == 1 and mc.labels[0, 50, 250] == 0 and mc.labels[0, 0, 0] == -1
