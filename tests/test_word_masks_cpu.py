"""Host-side checks of ``daam_word_masks``: the entry point in the header, the binding and the library; the machine code
of every kernel that was there before; the new kernels and their scratch use as the code object states it; and
``GlobalHeatMap.segment`` with ``engine.word_masks`` replaced by a recorder.  The kernels run in tests/test_gpu_word_masks.py."""
import json
import os
import re
import struct
import subprocess

import pytest
import torch

from oracle import fake_diffusers as fd
from test_tap_walk_cpu import PAIR_SHAS, WALK_SHAS, _kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KERNELS = ('word_masks_mean_kernel', 'word_masks_minmax_kernel', 'word_masks_out_kernel')


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    lib = build.build(verbose=False)
    return lib, build.kernel_shas(lib)


def test_entry_point_is_declared_bound_and_exported(built):
    from daam_amd import _native
    lib, _ = built
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'daam_hip.h')).read(), flags=re.S)
    assert re.search(r'DAAM_API int daam_word_masks\s*\(', header)
    assert re.search(r'#define DAAM_ABI_VERSION 6\b', header) and _native.ABI_VERSION == 6
    assert 'daam_word_masks' in _native.EXPORTS
    nm = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r' T daam_word_masks$', nm, flags=re.M)
    assert _native.load().daam_abi_version() == 6
    assert len(_native.load().daam_word_masks.argtypes) == 16


def test_old_kernels_untouched_and_new_ones_present(built):
    _, have = built
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'r06_counters.json')))['kernel_shas']
    assert len(rec) == 132
    assert {k: have.get(k) for k in rec} == rec
    assert {k: have.get(k) for k in PAIR_SHAS} == PAIR_SHAS
    assert {k: have.get(k) for k in WALK_SHAS} == WALK_SHAS
    for name in NEW_KERNELS:
        assert sum(name in k for k in have) == 1, name


def test_new_kernels_use_no_scratch(built):
    """Private segment size 0 and the private-segment enable bit clear in the kernel descriptors."""
    lib, have = built
    kds = _kernel_descriptors(lib)
    new = [k for k in have if any(name in k for name in NEW_KERNELS)]
    assert len(new) == 3 and all(k in kds for k in new)
    for k in new:
        private, = struct.unpack_from('<I', kds[k], 4)
        _, rsrc2 = struct.unpack_from('<II', kds[k], 48)
        assert private == 0 and not (rsrc2 & 1), (k, private)


# ------------------------------------------------------------------------------------------------
# GlobalHeatMap.segment
# ------------------------------------------------------------------------------------------------
class _Image:
    def __init__(self, width, height):
        self.size = (width, height)             # PIL order


PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


@pytest.fixture
def recorder(monkeypatch):
    from daam_amd import engine as E
    calls = []

    def word_masks(maps, idx_lists, out_h, out_w, absolute=False, threshold=0.4, labels=True):
        calls.append(dict(idx_lists=[list(i) for i in idx_lists], out=(out_h, out_w), absolute=absolute, threshold=threshold,
                          labels=labels))
        n = len(idx_lists)
        base = sum(len(c['idx_lists']) for c in calls[:-1])
        word_maps = torch.stack([torch.full(maps.shape[1:], float(base + j)) for j in range(n)])
        masks = torch.stack([torch.full((out_h, out_w), (base + j) % 251, dtype=torch.uint8) for j in range(n)])
        return word_maps, masks, torch.zeros(out_h, out_w, dtype=torch.uint8) if labels else None
    monkeypatch.setattr(E, 'word_masks', word_masks)
    return calls


def test_segment_resolves_words_and_sizes(recorder):
    from daam_amd import GlobalHeatMap, Segmentation, WordHeatMap
    from daam_amd.utils import compute_token_merge_indices
    tok = fd.FakeTokenizer()
    words = ['monkey', 'bicycle', ('photo', None), ('x', 3)]
    square = GlobalHeatMap(tok, PROMPT, torch.zeros(13, 8, 8))
    seg = square.segment(words, _Image(40, 24), threshold=0.3, absolute=True)
    want = [compute_token_merge_indices(tok, PROMPT, *((w, None) if isinstance(w, str) else w))[0] for w in words]
    assert want[:2] == [[5, 12], [8, 9]] and want[3] == [4]
    assert len(recorder) == 1 and recorder[0]['idx_lists'] == want
    assert recorder[0]['out'] == (40, 24)                  # square maps: (size[0], size[1]), the reference's order
    assert recorder[0]['threshold'] == 0.3 and recorder[0]['absolute'] is True and recorder[0]['labels'] is True
    assert isinstance(seg, Segmentation) and Segmentation.BACKGROUND == 255
    assert seg.words == ['monkey', 'bicycle', 'photo', 'x']
    assert all(isinstance(m, WordHeatMap) for m in seg.word_heat_maps)
    assert [m.word for m in seg.word_heat_maps] == seg.words and seg.word_heat_maps[3].word_idx == 3
    assert [float(m.heatmap[0, 0]) for m in seg.word_heat_maps] == [0.0, 1.0, 2.0, 3.0]
    assert seg.masks.shape == (4, 40, 24) and seg.labels.shape == (40, 24)
    assert torch.equal(seg.mask('bicycle'), seg.masks[1])
    with pytest.raises(KeyError):
        seg.mask('cat')
    host = seg.cpu()
    assert host.words == seg.words and torch.equal(host.masks, seg.masks) and torch.equal(host.labels, seg.labels)
    rect = GlobalHeatMap(tok, PROMPT, torch.zeros(13, 6, 10))
    rect.segment(['monkey'], _Image(40, 24))
    assert recorder[1]['out'] == (24, 40)                  # rectangular maps: [image height, image width]
    assert recorder[1]['threshold'] == 0.4 and recorder[1]['absolute'] is False


def test_segment_chunks_and_label_limit(recorder):
    from daam_amd import GlobalHeatMap
    tok = fd.FakeTokenizer()
    gm = GlobalHeatMap(tok, PROMPT, torch.zeros(13, 8, 8))
    words = [('w', i % 10) for i in range(70)]
    with pytest.raises(ValueError, match='32'):
        gm.segment(words, _Image(16, 16))
    assert not recorder
    gm.segment(words[:32], _Image(16, 16))
    assert [len(c['idx_lists']) for c in recorder] == [32] and recorder[0]['labels'] is True
    del recorder[:]
    seg = gm.segment(words, _Image(16, 16), labels=False)
    assert [len(c['idx_lists']) for c in recorder] == [32, 32, 6]
    assert all(c['labels'] is False for c in recorder)
    assert [i for c in recorder for i in c['idx_lists']] == [[i % 10 + 1] for i in range(70)]
    assert seg.labels is None and seg.masks.shape == (70, 16, 16) and len(seg.word_heat_maps) == 70
    assert [int(m[0, 0]) for m in seg.masks] == list(range(70))          # chunk order kept
    assert [float(m.heatmap[0, 0]) for m in seg.word_heat_maps] == [float(i) for i in range(70)]


def test_segment_unknown_word_raises(recorder):
    from daam_amd import GlobalHeatMap
    gm = GlobalHeatMap(fd.FakeTokenizer(), PROMPT, torch.zeros(13, 8, 8))
    with pytest.raises(ValueError, match='Search word cat not found in prompt!'):
        gm.segment(['monkey', 'cat'], _Image(16, 16))
    with pytest.raises(ValueError, match='Search word cat not found in prompt!'):
        gm.compute_word_heat_map('cat')
    assert not recorder


def test_engine_word_masks_checks_before_the_library(monkeypatch):
    """The ``_check_maps`` rules, the ``IndexError`` of ``word_heat_map`` and the per-call limits, none of which reach the library."""
    from daam_amd import engine as E
    monkeypatch.setattr(E.nat, 'load', lambda: pytest.fail('the library was reached'))
    with pytest.raises(RuntimeError, match='HIP device'):
        E.word_masks(torch.zeros(4, 8, 8), [[1]], 16, 16)
    with pytest.raises(RuntimeError, match='HIP device'):
        E.word_heat_map(torch.zeros(4, 8, 8), [1])
    monkeypatch.setattr(E, '_check_maps', lambda maps: None)
    with pytest.raises(IndexError, match='index 4 is out of bounds for dimension 0 with size 4'):
        E.word_masks(torch.zeros(4, 8, 8), [[1], [4]], 16, 16)
    for bad in ([], [[1]] * 33, [[1], []], [[1] * 128, [2] * 128]):
        with pytest.raises(ValueError):
            E.word_masks(torch.zeros(4, 8, 8), bad, 16, 16)
