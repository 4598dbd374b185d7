"""Host-side checks of ``daam_mask_overlap_matrix``: the entry point in the header, the binding, the library and the
integration guide; the new kernels in the code object, without scratch; the coercion of inputs and the 32 x 32 block tiling of
``evaluate.mask_overlap_matrix`` with the launcher replaced by numpy; the two ratios against ``evaluate._ratios``.  The kernel runs
in tests/test_gpu_mask_overlap_matrix.py."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from test_tap_walk_cpu import _kernel_descriptors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_KERNELS = ('mask_matrix_zero_kernel', 'mask_matrix_kernelILb0E', 'mask_matrix_kernelILb1E')


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    lib = build.build(verbose=False)
    return lib, build.kernel_shas(lib)


def test_entry_point_is_declared_bound_exported_and_documented(built):
    from daam_amd import _native
    import daam_amd
    lib, _ = built
    text = open(os.path.join(ROOT, 'include', 'daam_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'DAAM_API int daam_mask_overlap_matrix\s*\(', header)
    comment = text[:text.index('DAAM_API int daam_mask_overlap_matrix')].rsplit('/*', 1)[1]
    assert 'evaluate.py:14-35' in comment and 'heatmap.py:95-96' in comment
    assert re.search(r'#define DAAM_ABI_VERSION 6\b', header) and _native.ABI_VERSION == 6
    assert 'daam_mask_overlap_matrix' in _native.EXPORTS
    nm = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    assert re.search(r' T daam_mask_overlap_matrix$', nm, flags=re.M)
    assert len(_native.load().daam_mask_overlap_matrix.argtypes) == 10
    guide = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'lib.daam_mask_overlap_matrix.argtypes = [V, I, V, I, I, I, V, V, V, V]' in guide
    assert '| `daam_mask_overlap_matrix(a, n_a, b, n_b, h, w, inter, area_a, area_b, stream)` |' in guide
    assert 'daam_mask_matrix.hip' in build_sources()
    assert daam_amd.mask_overlap_matrix is daam_amd.evaluate.mask_overlap_matrix and daam_amd.MaskOverlaps is daam_amd.evaluate.MaskOverlaps


def build_sources():
    from daam_amd import build
    return build.SOURCES


def test_new_kernels_are_there_and_use_no_scratch(built):
    """Private segment size 0 and the private-segment enable bit clear in the kernel descriptors."""
    lib, have = built
    kds = _kernel_descriptors(lib)
    for name in NEW_KERNELS:
        match = [k for k in have if name in k]
        assert len(match) == 1 and match[0] in kds, name
        private, = struct.unpack_from('<I', kds[match[0]], 4)
        _, rsrc2 = struct.unpack_from('<II', kds[match[0]], 48)
        assert private == 0 and not (rsrc2 & 1), (name, private)


# ------------------------------------------------------------------------------------------------
# evaluate.mask_overlap_matrix on the host: coercion and tiling
# ------------------------------------------------------------------------------------------------
def _reference(a, b=None):
    a = np.asarray(a) != 0
    b = a if b is None else np.asarray(b) != 0
    inter = ((a[:, None] != 0) & (b[None] != 0)).sum((2, 3), dtype=np.int64)
    return inter, a.sum((1, 2), dtype=np.int64), b.sum((1, 2), dtype=np.int64)


@pytest.fixture
def numpy_launcher(monkeypatch):
    """The launch helper replaced by the numpy reference, and CPU tensors left where they are: what reaches the launcher is recorded."""
    from daam_amd import evaluate as ev
    calls = []

    def launch(a, b):
        assert a.dtype == torch.uint8 and a.dim() == 3 and a.is_contiguous() and 1 <= a.shape[0] <= 32
        assert b is None or (b.dtype == torch.uint8 and b.is_contiguous() and 1 <= b.shape[0] <= 32 and b.shape[1:] == a.shape[1:])
        calls.append((a, b))
        inter, area_a, area_b = _reference(a.numpy(), None if b is None else b.numpy())
        return tuple(torch.from_numpy(x.astype(np.int32)) for x in (inter, area_a, area_b))
    monkeypatch.setattr(ev, '_launch_overlap_matrix', launch)
    monkeypatch.setattr(ev, '_to_hip', lambda t, name, device=None: t)
    monkeypatch.setattr(ev.nat, 'load', lambda: pytest.fail('the library was reached'))
    return calls


def _stack(n, h, w, seed):
    return (np.random.default_rng(seed).random((n, h, w)) < 0.4).astype(np.uint8)


def _assert_counts(got, a, b=None):
    inter, area_a, area_b = _reference(a, b)
    assert got.intersection.dtype == torch.int32 and got.intersection.shape == inter.shape
    assert np.array_equal(got.intersection.numpy(), inter)
    assert np.array_equal(got.area_a.numpy(), area_a) and np.array_equal(got.area_b.numpy(), area_b)


def test_blocks_of_32_are_stitched(numpy_launcher):
    from daam_amd.evaluate import mask_overlap_matrix
    a, b = _stack(33, 5, 7, 1), _stack(70, 5, 7, 2)
    _assert_counts(mask_overlap_matrix(torch.from_numpy(a), torch.from_numpy(b)), a, b)
    assert [(x.shape[0], y.shape[0]) for x, y in numpy_launcher] == [(32, 32), (32, 32), (32, 6), (1, 32), (1, 32), (1, 6)]
    del numpy_launcher[:]
    _assert_counts(mask_overlap_matrix(torch.from_numpy(a[:32]), torch.from_numpy(b[:32])), a[:32], b[:32])
    assert len(numpy_launcher) == 1


def test_one_stack_of_more_than_32(numpy_launcher):
    """Diagonal blocks are one-stack calls, a block above the diagonal is a two-stack call and serves the one below it too."""
    from daam_amd.evaluate import mask_overlap_matrix
    a = _stack(70, 4, 9, 3)
    got = mask_overlap_matrix(torch.from_numpy(a))
    _assert_counts(got, a)
    assert [(x.shape[0], None if y is None else y.shape[0]) for x, y in numpy_launcher] == \
        [(32, None), (32, 32), (32, 6), (32, None), (32, 6), (6, None)]
    assert torch.equal(got.intersection, got.intersection.t()) and torch.equal(got.intersection.diagonal(), got.area_a)
    del numpy_launcher[:]
    _assert_counts(mask_overlap_matrix(torch.from_numpy(a[:7])), a[:7])
    assert len(numpy_launcher) == 1 and numpy_launcher[0][1] is None


def test_input_coercion(numpy_launcher):
    from daam_amd.evaluate import mask_overlap_matrix
    a, b = _stack(3, 6, 5, 4), _stack(2, 6, 5, 5)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    got = mask_overlap_matrix(ta, tb)
    assert numpy_launcher[-1][0].data_ptr() == ta.data_ptr()                     # uint8 goes through as it is
    _assert_counts(got, a, b)
    as_bool = ta.bool()
    _assert_counts(mask_overlap_matrix(as_bool, tb.bool()), a, b)
    assert numpy_launcher[-1][0].data_ptr() == as_bool.data_ptr()                # and so does bool, as its bytes
    for dtype in (torch.float32, torch.float16, torch.int64):
        _assert_counts(mask_overlap_matrix(ta.to(dtype) * 3, tb.to(dtype)), a, b)
    _assert_counts(mask_overlap_matrix(ta.float() * -0.5, tb * 255), a, b)       # any non-zero value is set
    _assert_counts(mask_overlap_matrix(ta[0], tb), a[:1], b)                     # [h, w] is one mask
    _assert_counts(mask_overlap_matrix(ta, tb[1]), a, b[1:])
    wide = torch.from_numpy(np.ascontiguousarray(np.repeat(a, 2, axis=2)))
    _assert_counts(mask_overlap_matrix(wide[:, :, ::2], tb), a, b)               # a strided view is made contiguous
    n_calls = len(numpy_launcher)
    with pytest.raises(ValueError, match='does not resize'):
        mask_overlap_matrix(ta, torch.zeros(2, 5, 6, dtype=torch.uint8))
    with pytest.raises(ValueError):
        mask_overlap_matrix(torch.zeros(2, 2, 6, 5, dtype=torch.uint8))
    with pytest.raises(ValueError):
        mask_overlap_matrix(torch.zeros(0, 6, 5, dtype=torch.uint8))
    assert len(numpy_launcher) == n_calls


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the no-GPU failure mode')
def test_cpu_masks_without_a_device_fail_loudly():
    from daam_amd.evaluate import mask_overlap_matrix
    with pytest.raises(RuntimeError, match='no HIP device'):
        mask_overlap_matrix(torch.zeros(2, 4, 4, dtype=torch.uint8))


def test_ratios_follow_the_pair_route():
    """``iou`` / ``ioa`` on hand-made counts against ``_ratios`` on the same counts as fp32 sums, bit for bit."""
    from daam_amd.evaluate import MaskOverlaps, _ratios
    inter = torch.tensor([[0, 3, 7], [1, 0, 1000003]], dtype=torch.int32)
    area_a = torch.tensor([0, 1000003], dtype=torch.int32)
    area_b = torch.tensor([5, 0, 16777215], dtype=torch.int32)
    inter[0] = 0                                                                 # a[0] is empty
    ov = MaskOverlaps(inter, area_a, area_b)
    iou, ioa = ov.iou(), ov.ioa()
    assert iou.dtype == torch.float32 and ioa.dtype == torch.float32 and iou.shape == (2, 3) and ioa.shape == (2, 3)
    sums = torch.stack([torch.tensor([float(inter[i, j]), float(area_a[i]), float(area_b[j])]) for i in range(2) for j in range(3)])
    want_iou, want_ioa = _ratios(sums)
    assert np.array_equal(iou.numpy().reshape(-1), want_iou) and np.array_equal(ioa.numpy().reshape(-1), want_ioa)
    assert iou[0, 0] == 0.0 and ioa[0, 0] == 0.0 and iou[1, 2] > 0.0
    host = ov.cpu()
    assert torch.equal(host.intersection, inter) and torch.equal(host.area_a, area_a) and torch.equal(host.area_b, area_b)


def test_segmentation_scores_go_through_the_matrix_route(numpy_launcher):
    from daam_amd import Segmentation, WordHeatMap
    masks = torch.from_numpy(_stack(3, 8, 8, 6))
    seg = Segmentation(['x', 'y', 'z'], [WordHeatMap(torch.zeros(4, 4), w) for w in 'xyz'], masks, None)
    _assert_counts(seg.overlaps(), masks.numpy())
    truth = torch.from_numpy(_stack(2, 8, 8, 7))
    _assert_counts(seg.overlaps(truth), masks.numpy(), truth.numpy())
    other = Segmentation(['t', 'u'], [], truth, None)
    assert torch.equal(seg.iou(other), seg.overlaps(truth).iou()) and seg.iou(truth).shape == (3, 2)
    assert torch.equal(seg.ioa(), seg.overlaps().ioa())
    inter, area, _ = _reference(masks.numpy())
    assert seg.ioa_of('x', 'z') == float(np.float32(inter[0, 2]) / (np.float32(area[0]) + np.float32(1e-8)))
    with pytest.raises(KeyError):
        seg.ioa_of('x', 'w')
