"""``daam_region_scores`` on the device against the float64 oracle of ``tests/_region_domain.py``, which derives the
bound ``ulp(want) + g_K S`` and counts K; ``tests/test_region_scores_cpu.py`` holds the oracle, the bound and the cases to what this
file relies on.  Every bound case goes through the C ABI with guard bytes around every output; the stacks of 33 and the API checks
go through Python.

Worst |got - want| / bound measured on gfx950 over all bound cases: see DESIGN 3.13."""
import functools

import numpy as np
import pytest
import torch

import _epilogue_domain as ed
import _region_domain as rd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
E_INVALID = -1


@functools.lru_cache(maxsize=None)
def _case(sizes, n, first):
    (h, w), (H, W) = sizes
    masks, maps = rd.mask_stack(H, W, n, first), rd.map_sets(h, w)
    return masks, maps, rd.oracle(masks, maps, h, w)


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _raw(masks, maps, h, w, byte_offset=0, dots=True):
    """One call through the C ABI.  ``masks`` uint8 numpy [M, H, W], ``maps`` f32 numpy [G, rows, h, w].  Returns numpy
    ``(scores [G, M, rows], area [M], footprint [M, h, w])`` after checking the guard elements around every output."""
    from daam_amd import _native as nat
    lib = nat.load()
    M, H, W = masks.shape
    G, rows = maps.shape[:2]
    raw = torch.zeros(masks.size + byte_offset + 16, dtype=torch.uint8, device=DEV)
    dev_masks = raw[byte_offset:byte_offset + masks.size]
    dev_masks.copy_(torch.from_numpy(masks.reshape(-1)))
    dev_maps = torch.from_numpy(np.ascontiguousarray(maps)).to(DEV)
    s_buf, scores = _guarded(G * M * rows, torch.float32, -7.0)
    f_buf, foot = _guarded(M * h * w, torch.float32, -7.0)
    a_buf, area = _guarded(M, torch.int32, -7)
    size = lib.daam_region_scores_workspace(M, H, W, h, w)
    assert size > 0
    w_buf, ws = _guarded(size, torch.uint8, 0x5a)
    assert ws.data_ptr() % 16 == 0
    nat.check(lib.daam_region_scores(dev_masks.data_ptr(), M, H, W, dev_maps.data_ptr() if dots else None, G, rows, h, w, foot.data_ptr(),
                                     scores.data_ptr() if dots else None, area.data_ptr(), ws.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for buf, fill in ((s_buf, -7.0), (f_buf, -7.0), (a_buf, -7), (w_buf, 0x5a)):
        host = buf.cpu()
        assert (host[:GUARD] == fill).all() and (host[-GUARD:] == fill).all(), 'guard bytes overwritten'
    if not dots:
        assert (s_buf.cpu() == -7.0).all()
    return scores.cpu().numpy().reshape(G, M, rows), area.cpu().numpy().astype(np.int64), foot.cpu().numpy().reshape(M, h, w)


@functools.lru_cache(maxsize=None)
def _got(sizes, n, first):
    masks, maps, _ = _case(sizes, n, first)
    return _raw(masks, maps, *sizes[0])


@pytest.mark.parametrize('case', list(rd.cases()), ids=str)
def test_scores_meet_the_bound(case):
    sizes, n, first = case
    masks, maps, ref = _case(*case)
    scores, area, foot = _got(*case)
    assert ref['K'] * rd.U <= rd.CAP
    ratio = rd.worst(scores, ref)
    print(f'{case}: K = {ref["K"]}, worst |got - want| / bound = {ratio:.4f}')
    assert np.isfinite(scores).all() and ratio <= 1.0, ratio
    assert (area == ref['area']).all()
    kinds = rd.stack_kinds(n, first)
    clear = [i for i, k in enumerate(kinds) if k == 'all_clear']
    assert (scores[:, clear] == 0.0).all() and (area[clear] == 0).all()
    assert (scores[-1, :, rd.ZERO_ROW] == 0.0).all(), 'a zero row leaks'
    if sizes[0] == sizes[1]:
        assert np.array_equal(foot, (masks != 0).astype(np.float32)), 'identity sizes: the footprint is the mask'
    # set bytes of 255 and of 2 count like 1
    for name in ('random255', 'random2'):
        for i in [i for i, k in enumerate(kinds) if k == name]:
            twin = [j for j, k in enumerate(kinds) if k == 'random' and j // len(rd.MASK_KINDS) == i // len(rd.MASK_KINDS)]
            if twin:
                assert np.array_equal(scores[:, i], scores[:, twin[0]]) and np.array_equal(foot[i], foot[twin[0]]) and area[i] == area[twin[0]]


@pytest.mark.parametrize('sizes', [s for s in rd.SIZE_SETS if s != rd.LONG], ids=str)
def test_area_is_the_overlap_matrix_area(sizes):
    from daam_amd.evaluate import mask_overlap_matrix
    masks, _, _ = _case(sizes, 32, 0)
    _, area, _ = _got(sizes, 32, 0)
    assert np.array_equal(area, mask_overlap_matrix(torch.from_numpy(masks).to(DEV)).area_a.cpu().numpy())


@pytest.mark.parametrize('sizes', [rd.SIZE_SETS[0], rd.SIZE_SETS[1], rd.SIZE_SETS[2], rd.SIZE_SETS[4]], ids=str)
def test_bit_equal_runs_stacks_and_sets(sizes):
    """Two runs agree bit for bit; a mask scored alone (its plane starting elsewhere in memory) gives the bits it gives inside a stack
    of 32 and inside a stack of 33 (Python's chunks of 32 + 1); three sets in one call give the bits of three calls."""
    from daam_amd import engine
    (h, w), (H, W) = sizes
    masks, maps, _ = _case(sizes, 32, 0)
    scores, area, foot = _got(sizes, 32, 0)
    again = _raw(masks, maps, h, w)
    assert all(np.array_equal(a, b) for a, b in zip(again, (scores, area, foot)))
    for m, offset in ((0, 1), (7, 0), (9, 5), (31, 3)):
        s1, a1, f1 = _raw(masks[m:m + 1], maps, h, w, byte_offset=offset)
        assert np.array_equal(s1[:, 0], scores[:, m]) and a1[0] == area[m] and np.array_equal(f1[0], foot[m]), m
    more = np.concatenate([masks, masks[9:10]])
    s33, a33, f33 = engine.region_scores(torch.from_numpy(maps).to(DEV), torch.from_numpy(more))
    assert s33.shape == (maps.shape[0], 33, rd.ROWS) and a33.dtype == torch.int32 and f33.shape == (33, h, w)
    assert np.array_equal(s33.cpu().numpy()[:, :32], scores) and np.array_equal(s33.cpu().numpy()[:, 32], scores[:, 9])
    assert np.array_equal(f33.cpu().numpy()[:32], foot) and np.array_equal(f33.cpu().numpy()[32], foot[9])
    assert np.array_equal(a33.cpu().numpy()[:32], area) and a33[32].item() == area[9]
    for g in range(3):
        one = _raw(masks, maps[g:g + 1], h, w)[0]
        assert np.array_equal(one[0], scores[g])
    # the footprint and the area alone, and further sets against the kept footprint
    _, a0, f0 = _raw(masks, maps, h, w, dots=False)
    assert np.array_equal(a0, area) and np.array_equal(f0, foot)
    dots = engine.region_dots(torch.from_numpy(maps).to(DEV), torch.from_numpy(foot).to(DEV))
    assert np.array_equal(dots.cpu().numpy(), scores)
    # bool masks, and a single [H, W] mask against one [rows, h, w] set
    s2, a2, _ = engine.region_scores(torch.from_numpy(maps[1]).to(DEV), torch.from_numpy(masks[0] != 0).to(DEV))
    assert s2.shape == (1, rd.ROWS) and np.array_equal(s2.cpu().numpy()[0], scores[1, 0]) and a2.item() == area[0]


@pytest.mark.parametrize('sizes', [rd.SIZE_SETS[0], rd.SIZE_SETS[2]], ids=str)
def test_cross_route_expand_then_sum(sizes):
    """expand_word_map(absolute=True) on the device, summed under each mask in float64 on the host, against the scores: within this
    file's bound plus the resize bound 8 u S of the epilogue domain (every pixel's value carries at most eight roundings)."""
    from daam_amd import engine
    (h, w), (H, W) = sizes
    masks, maps, ref = _case(sizes, 32, 0)
    scores, _, _ = _got(sizes, 32, 0)
    bits = (masks != 0).astype(np.float64)
    for g in range(maps.shape[0]):
        for t in range(rd.ROWS):
            big = engine.expand_word_map(torch.from_numpy(maps[g, t]).to(DEV), H, W, absolute=True).cpu().numpy().astype(np.float64)
            other = (bits * big[None]).sum((1, 2))
            tol = ref['bound'][g, :, t] + ed.K_RESIZE * ref['mag'][g, :, t]
            assert (np.abs(other - scores[g, :, t]) <= tol).all(), (g, t)


def test_invalid_arguments():
    from daam_amd import _native as nat
    lib = nat.load()
    ok = dict(n_masks=2, H=16, W=16, n_sets=1, rows=3, h=8, w=8)
    masks = torch.zeros(2 * 16 * 16, dtype=torch.uint8, device=DEV)
    maps = torch.zeros(3 * 8 * 8, dtype=torch.float32, device=DEV)
    foot, scores, area = (torch.zeros(256, dtype=torch.float32, device=DEV), torch.zeros(16, dtype=torch.float32, device=DEV),
                          torch.zeros(4, dtype=torch.int32, device=DEV))
    ws = torch.zeros(lib.daam_region_scores_workspace(2, 16, 16, 8, 8), dtype=torch.uint8, device=DEV)

    def call(maps_ptr=maps.data_ptr(), scores_ptr=scores.data_ptr(), **change):
        a = dict(ok, **change)
        return lib.daam_region_scores(masks.data_ptr(), a['n_masks'], a['H'], a['W'], maps_ptr, a['n_sets'], a['rows'], a['h'], a['w'],
                                      foot.data_ptr(), scores_ptr, area.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert call() == 0
    for change in (dict(n_masks=0), dict(n_masks=33), dict(h=0), dict(h=129), dict(w=0), dict(w=129), dict(H=0), dict(W=0),
                   dict(H=65536, W=32768), dict(n_sets=0), dict(rows=0)):
        assert call(**change) == E_INVALID, change
        if not {'n_sets', 'rows'} & set(change):
            a = dict(ok, **change)
            assert lib.daam_region_scores_workspace(a['n_masks'], a['H'], a['W'], a['h'], a['w']) == 0, change
    assert call(maps_ptr=None) == E_INVALID and call(scores_ptr=None) == E_INVALID
    assert call(maps_ptr=None, scores_ptr=None) == 0
    torch.cuda.synchronize()
    assert (scores == 0).all() and (area == 0).all() and (foot == 0).all()


# ------------------------------------------------------------------------------------------------
# GlobalHeatMap.attribute
# ------------------------------------------------------------------------------------------------
class _Image:
    def __init__(self, width, height):
        self.size = (width, height)


PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'
WORDS = ['monkey', 'bicycle', 'photo']


def test_attribute_a_segmentation():
    from daam_amd import GlobalHeatMap, RegionAttribution, engine
    from daam_amd.utils import compute_token_merge_indices
    from oracle import fake_diffusers as fd
    tok = fd.FakeTokenizer()
    maps = ed.planes('real', 13, 64, 64, seed=5)
    ghm = GlobalHeatMap(tok, PROMPT, torch.from_numpy(maps).to(DEV))
    seg = ghm.segment(WORDS, _Image(96, 96), threshold=0.3)
    att = ghm.attribute(seg)
    assert isinstance(att, RegionAttribution) and att.scores.device.type == 'cuda'
    scores, area, foot = engine.region_scores(ghm.heat_maps, seg.masks)
    assert torch.equal(att.scores, scores) and torch.equal(att.area, area) and torch.equal(att.footprint, foot)
    assert att.scores.shape == (3, 13) and torch.equal(att.mean(), scores / area.clamp(min=1).float()[:, None])
    assert torch.equal(ghm.attribute(seg.masks[1]).scores[0], scores[1])
    host = att.cpu()
    assert host.scores.device.type == 'cpu' and torch.equal(host.scores, scores.cpu())

    masks = seg.masks.cpu().numpy()
    ref = rd.oracle(masks, maps[None], 64, 64)
    assert rd.worst(scores.cpu().numpy()[None], ref) <= 1.0
    # word_scores against the score of the word's own mean plane: each within its bound of its float64 value, and the two
    # float64 values apart by the word mean's (n + 1) u of sum F_abs mean|v|
    per_word = att.word_scores(WORDS).cpu().numpy().astype(np.float64)
    wants, bounds = [], []
    for col, word in enumerate(WORDS):
        idxs, _ = compute_token_merge_indices(tok, PROMPT, word, None)
        n = len(idxs)
        plane = ghm.compute_word_heat_map(word).heatmap
        single = GlobalHeatMap(tok, PROMPT, plane[None].contiguous()).attribute(seg).scores[:, 0].cpu().numpy().astype(np.float64)
        ref_single = rd.oracle(masks, plane.cpu().numpy()[None, None], 64, 64)
        b_single = ref_single['bound'][0, :, 0]
        mean_mag = ref['mag'][0][:, idxs].mean(1)
        b_mean = ref['bound'][0][:, idxs].mean(1) + 2 * (n + 1) * rd.U * mean_mag
        assert (np.abs(per_word[:, col] - single) <= b_single + b_mean).all(), word
        wants.append(ref['want'][0][:, idxs].mean(1))
        bounds.append(b_mean)
    wants, bounds = np.stack(wants, 1), np.stack(bounds, 1)
    values, index = att.top_words(WORDS, k=1)
    for m in range(3):
        order = np.argsort(-wants[m])
        if wants[m, order[0]] - wants[m, order[1]] > bounds[m, order[0]] + bounds[m, order[1]]:
            assert index[m, 0].item() == order[0] and values[m, 0].item() == np.float32(per_word[m, order[0]])
