"""``daam_word_masks`` on the device: masks and a label map for many words in three launches.

The batched kernels restate the arithmetic of the single-word kernels, so every comparison with them is exact (``torch.equal``):
``word_maps[j]`` against ``word_heat_map``, ``masks[j]`` against ``expand_word_map(threshold=)`` and the labels against the arg-max
rule evaluated in torch on the single-word f32 planes.  The single-word kernels themselves are held to the numpy oracle by
``test_gpu_parity.py::test_normalize_and_word_maps``; ``test_masks_against_the_oracle`` repeats that for the masks on its inputs.

One departure from the letter of the issue: with ``threshold=0.0`` the single-word call returns the values themselves, and its
reference mask is taken as ``> 0`` (the rule ``v > threshold`` the entry point documents), not ``!= 0``: an ``absolute`` bicubic plane
undershoots below zero next to a steep edge, and ``!= 0`` would count those pixels."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import heatmap_oracle as ho

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

ROWS = 16                      # planes 14 and 15 are all zero
# source -> output: identity branch, upscale, row tails at a non-integer scale, downscale, rectangular sources, a tiny one
CASES = [((64, 64), (64, 64)), ((64, 64), (128, 128)), ((64, 64), (70, 67)), ((64, 64), (48, 48)), ((52, 76), (104, 152)),
         ((52, 76), (83, 121)), ((6, 10), (24, 40))]


def _maps(h, w, seed=11):
    rng = np.random.default_rng(seed)
    maps = np.abs(rng.standard_normal((ROWS, h, w))).astype(np.float32)
    maps[14:] = 0
    return torch.from_numpy(maps).to(DEV)


def _words(n):
    """A three-token word, a word sharing plane 3 with it, a word of all-zero planes; then two identical words and random ones."""
    words = [[1, 2, 3], [3, 4], [14, 15], [5], [5]]
    rng = np.random.default_rng(n)
    while len(words) < n:
        words.append([int(i) for i in rng.integers(0, 14, size=int(rng.integers(1, 5)))])
    return words[:n]


def _single(maps, words, out, absolute, threshold):
    """Per word, from the single-word kernels: the mean plane, the f32 expanded plane and the mask at ``threshold``."""
    from daam_amd import engine as E
    means = [E.word_heat_map(maps, idxs) for idxs in words]
    values = torch.stack([E.expand_word_map(m, out[0], out[1], absolute=absolute) for m in means])
    thresholded = torch.stack([E.expand_word_map(m, out[0], out[1], absolute=absolute, threshold=threshold) for m in means])
    masks = thresholded != 0 if threshold else thresholded > 0
    return torch.stack(means), values, masks.to(torch.uint8)


def _label_rule(values, threshold):
    """The smallest j with v_j = max_j v_j where that maximum is > threshold, else 255."""
    top = values.max(0).values
    j = torch.arange(values.shape[0], device=values.device).view(-1, 1, 1)
    first = torch.where(values == top, j, values.shape[0]).min(0).values
    return torch.where(top > threshold, first, 255).to(torch.uint8)


def _check(maps, words, out, absolute, threshold):
    from daam_amd import engine as E
    word_maps, masks, labels = E.word_masks(maps, words, out[0], out[1], absolute=absolute, threshold=threshold)
    means, values, want = _single(maps, words, out, absolute, threshold)
    assert torch.equal(word_maps, means)
    assert masks.dtype == torch.uint8 and labels.dtype == torch.uint8
    diff = int((masks != want).sum())
    print(f'{tuple(maps.shape[1:])}->{out} W={len(words)} absolute={absolute} t={threshold}: {diff} mask elements differ, '
          f'{int((labels != _label_rule(values, threshold)).sum())} labels differ')
    assert torch.equal(masks, want)
    assert torch.equal(labels, _label_rule(values, threshold))
    if len(words) >= 3:                     # the all-zero word: an empty mask, never a label
        assert not masks[2].any() and not (labels == 2).any()
    if len(words) >= 5:                     # words 3 and 4 are the same planes: every pixel a tie, the lower index wins
        assert torch.equal(masks[3], masks[4]) and not (labels == 4).any()
    return masks, labels


@pytest.mark.parametrize('n_words', [1, 3, 32])
@pytest.mark.parametrize('src,out', CASES)
def test_bit_identical_to_the_single_word_kernels(src, out, n_words):
    maps = _maps(*src)
    words = _words(n_words)
    for absolute in (False, True):
        for threshold in (0.4, 0.0):
            _check(maps, words, out, absolute, threshold)


def test_ten_words_at_1024():
    masks, labels = _check(_maps(64, 64), _words(10), (1024, 1024), False, 0.4)
    assert masks.shape == (10, 1024, 1024) and labels.shape == (1024, 1024)


def test_ties_and_background():
    """Two identical index lists: every pixel is a tie and goes to the lower index.  A threshold above every value: all background."""
    from daam_amd import engine as E
    maps = _maps(64, 64)
    _, masks, labels = E.word_masks(maps, [[7, 8], [7, 8]], 96, 96, threshold=0.0)
    assert masks[0].any() and torch.equal(masks[0], masks[1])
    assert set(labels.unique().tolist()) <= {0, 255} and (labels == 0).any()
    assert torch.equal(labels == 0, masks[0] != 0)
    for absolute, threshold in ((False, 1.5), (True, 1e6)):
        _, masks, labels = E.word_masks(maps, _words(5), 96, 96, absolute=absolute, threshold=threshold)
        assert not masks.any() and bool((labels == 255).all())


def test_masks_against_the_oracle():
    """Inputs and sizes of test_normalize_and_word_maps.  A mask element may differ from the oracle's only where the oracle's value is
    within 2e-5 (that test's value tolerance) of the threshold; the oracle alone first shows that few elements are that close."""
    from daam_amd import engine as E
    rng = np.random.default_rng(5)
    maps = np.abs(rng.standard_normal((9, 64, 64))).astype(np.float32)
    words = [[2, 3, 5], [1], [4, 6]]
    gm = torch.from_numpy(maps).to(DEV)
    threshold = 0.4
    for size in (64, 128, 512):
        for absolute in (False, True):
            want = np.stack([ho.expand_as(ho.word_heat_map(maps, idxs), size, absolute=absolute) for idxs in words])
            near = np.abs(want - np.float32(threshold)) <= 2e-5
            assert near.mean() <= 1e-3
            word_maps, masks, _ = E.word_masks(gm, words, size, size, absolute=absolute, threshold=threshold)
            np.testing.assert_allclose(word_maps.cpu().numpy(), np.stack([ho.word_heat_map(maps, i) for i in words]), rtol=1e-6, atol=1e-7)
            differ = masks.cpu().numpy() != (want > threshold)
            print(f'size {size} absolute={absolute}: {int(near.sum())} near the threshold, {int(differ.sum())} differ')
            assert not (differ & ~near).any()


def _raw(maps, idx, begin, n_words, word_maps, out_h, out_w, absolute, threshold, masks, labels, ws, rows=None):
    from daam_amd import _native as nat
    rows = maps.shape[0] if rows is None else rows
    ptr = lambda t: None if t is None else t.data_ptr()
    return nat.load().daam_word_masks(maps.data_ptr(), rows, maps.shape[1], maps.shape[2], (ctypes.c_int32 * max(len(idx), 1))(*idx),
                                      (ctypes.c_int32 * len(begin))(*begin), n_words, ptr(word_maps), out_h, out_w, int(absolute),
                                      threshold, ptr(masks), ptr(labels), ptr(ws), torch.cuda.current_stream().cuda_stream)


def _buffers(n, h, w, out_h, out_w, fill=7):
    return (torch.full((n, h, w), float(fill), device=DEV), torch.full((n, out_h, out_w), fill, dtype=torch.uint8, device=DEV),
            torch.full((out_h, out_w), fill, dtype=torch.uint8, device=DEV), torch.empty(64, device=DEV))


def test_null_masks_or_labels():
    from daam_amd import engine as E
    maps = _maps(52, 76)
    words = _words(3)
    idx, begin = [i for w in words for i in w], [0, 3, 5, 7]
    _, want_masks, want_labels = E.word_masks(maps, words, 83, 121)
    wm, masks, labels, ws = _buffers(3, 52, 76, 83, 121)
    assert _raw(maps, idx, begin, 3, wm, 83, 121, False, 0.4, None, labels, ws) == 0
    assert torch.equal(labels, want_labels) and bool((masks == 7).all())
    wm, masks, labels, ws = _buffers(3, 52, 76, 83, 121)
    assert _raw(maps, idx, begin, 3, wm, 83, 121, False, 0.4, masks, None, ws) == 0
    assert torch.equal(masks, want_masks) and bool((labels == 7).all())


@pytest.mark.parametrize('name,idx,begin,n_words', [
    ('no words', [1], [0, 1], 0),
    ('33 words', list(range(14)) * 3, list(range(34)), 33),
    ('an empty word', [1, 2], [0, 2, 2], 2),
    ('an index equal to rows', [1, ROWS], [0, 1, 2], 2),
    ('256 indices', [1] * 256, [0, 128, 256], 2),
])
def test_bad_arguments(name, idx, begin, n_words):
    from daam_amd import _native as nat
    maps = _maps(6, 10)
    wm, masks, labels, ws = _buffers(33, 6, 10, 24, 40)
    assert _raw(maps, idx, begin, n_words, wm, 24, 40, False, 0.4, masks, labels, ws) == nat.E_INVALID, name
    torch.cuda.synchronize()
    assert bool((wm == 7).all()) and bool((masks == 7).all()) and bool((labels == 7).all())


def test_second_call_on_the_stream():
    """The min / max pairs are started anew by every call: other words through the same workspace give their own results."""
    maps = _maps(64, 64)
    wm, masks, labels, ws = _buffers(2, 64, 64, 128, 128)
    for words in ([[1, 2, 3], [6]], [[14], [9, 10]]):
        idx, begin = [i for w in words for i in w], [0, len(words[0]), len(words[0]) + len(words[1])]
        assert _raw(maps, idx, begin, 2, wm, 128, 128, False, 0.4, masks, labels, ws) == 0
        means, values, want = _single(maps, words, (128, 128), False, 0.4)
        assert torch.equal(wm, means) and torch.equal(masks, want) and torch.equal(labels, _label_rule(values, 0.4))
