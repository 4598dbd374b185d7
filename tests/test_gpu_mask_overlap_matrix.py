"""``daam_mask_overlap_matrix`` on the device: the intersection matrix of two stacks of u8 masks and their areas.

Everything is integer, so every comparison is exact: the reference is ``(a[:, None] != 0) & (b[None] != 0)`` summed over the pixels
in numpy.  The ratios are held bit for bit to ``compute_iou`` / ``compute_ioa`` (the pair route): both divide exactly representable
counts in IEEE fp32 in one operand order."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SHAPES = [(1, 1), (1, 3), (3, 5), (7, 9), (1, 64), (5, 13), (64, 64), (33, 130), (63, 65), (256, 256), (104, 152)]
COUNTS = [(1, 1), (3, 2), (32, 32), (32, 1), (5, 32)]
DENSITIES = (0.0, 0.03, 0.5, 1.0)


def _reference(a, b=None):
    a = np.asarray(a) != 0
    b = a if b is None else np.asarray(b) != 0
    a2, b2 = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    inter = np.stack([(a2[i][None] & b2).sum(1, dtype=np.int64) for i in range(a2.shape[0])])
    return inter, a2.sum(1, dtype=np.int64), b2.sum(1, dtype=np.int64)


def _masks(n, h, w, seed):
    """Bernoulli planes, the density of each drawn from DENSITIES by the seed."""
    rng = np.random.default_rng(seed)
    return np.stack([(rng.random((h, w)) < DENSITIES[int(rng.integers(4))]) for _ in range(n)]).astype(np.uint8)


def _dense(n, h, w, seed, density=0.4):
    rng = np.random.default_rng(seed)
    return (rng.random((n, h, w)) < density).astype(np.uint8)


def _assert_exact(got, a, b=None):
    inter, area_a, area_b = _reference(a, b)
    assert got.intersection.dtype == torch.int32 and got.area_a.dtype == torch.int32 and got.area_b.dtype == torch.int32
    assert got.intersection.device.type == 'cuda'
    assert torch.equal(got.intersection.cpu().long(), torch.from_numpy(inter))
    assert torch.equal(got.area_a.cpu().long(), torch.from_numpy(area_a))
    assert torch.equal(got.area_b.cpu().long(), torch.from_numpy(area_b))


@pytest.mark.parametrize('n_a,n_b', COUNTS)
@pytest.mark.parametrize('h,w', SHAPES)
def test_exact(h, w, n_a, n_b):
    from daam_amd.evaluate import mask_overlap_matrix
    a, b = _masks(n_a, h, w, 100 * h + w), _masks(n_b, h, w, 100 * h + w + 7)
    _assert_exact(mask_overlap_matrix(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)), a, b)


@pytest.mark.parametrize('h,w,n', [(1024, 1024, 32), (832, 1216, 10)])
def test_exact_at_image_size(h, w, n):
    from daam_amd.evaluate import mask_overlap_matrix
    a, b = _masks(n, h, w, 1), _masks(n, h, w, 2)
    _assert_exact(mask_overlap_matrix(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)), a, b)


def test_byte_semantics():
    from daam_amd.evaluate import mask_overlap_matrix
    rng = np.random.default_rng(3)
    values = np.array([0, 1, 2, 128, 255], dtype=np.uint8)
    a = values[rng.integers(0, 5, size=(5, 33, 130))]
    b = values[rng.integers(0, 5, size=(4, 33, 130))]
    a[0, 0, :5] = values                              # all five side by side
    b[0, 0, :5] = values[::-1]
    got = mask_overlap_matrix(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    _assert_exact(got, a, b)
    as_bool = mask_overlap_matrix(torch.from_numpy(a != 0).to(DEV), torch.from_numpy(b != 0).to(DEV))
    as_u8 = mask_overlap_matrix(torch.from_numpy(a != 0).to(DEV).view(torch.uint8), torch.from_numpy(b != 0).to(DEV).view(torch.uint8))
    for name in ('intersection', 'area_a', 'area_b'):
        assert torch.equal(getattr(as_bool, name), getattr(as_u8, name)) and torch.equal(getattr(as_bool, name), getattr(got, name))
    as_float = mask_overlap_matrix(torch.from_numpy(a).to(DEV).float() * 0.25, torch.from_numpy(b).to(DEV).to(torch.int64))
    assert torch.equal(as_float.intersection, got.intersection)


@pytest.mark.parametrize('offset', [1, 2, 3])
@pytest.mark.parametrize('h,w,n', [(7, 9, 5), (63, 65, 4), (33, 131, 32)])
def test_unaligned_stacks_and_guard_bytes(offset, h, w, n):
    """The stack starts ``offset`` bytes into a buffer and h * w is odd: every plane starts at another residue mod 4 (and mod 16).
    The bytes directly before and after the stack are 255 and must not be counted."""
    from daam_amd.evaluate import mask_overlap_matrix
    assert (h * w) % 2 == 1
    a, b = _masks(n, h, w, offset), _masks(3, h, w, offset + 10)
    a[:, 0, 0] = 1                                     # the first and the last pixel of every plane count
    a[:, -1, -1] = 1
    b[:, 0, 0] = 1
    b[:, -1, -1] = 1

    def place(m, k):
        buf = torch.full((k + m.size + 64,), 255, dtype=torch.uint8, device=DEV)
        buf[k:k + m.size] = torch.from_numpy(m.reshape(-1)).to(DEV)
        view = buf[k:k + m.size].view(m.shape)
        assert view.data_ptr() % 4 == k % 4 and view.is_contiguous()
        return view
    _assert_exact(mask_overlap_matrix(place(a, offset), place(b, 16 + (offset + 1) % 4)), a, b)
    _assert_exact(mask_overlap_matrix(place(a, offset)), a)


def _raw(a, n_a, b, n_b, h, w, inter, area_a, area_b):
    from daam_amd import _native as nat
    ptr = lambda t: None if t is None else t.data_ptr()
    return nat.load().daam_mask_overlap_matrix(ptr(a), n_a, ptr(b), n_b, h, w, ptr(inter), ptr(area_a), ptr(area_b),
                                               torch.cuda.current_stream().cuda_stream)


FILL = 0x7fffffff


def test_outputs_are_owned_by_the_call():
    inter = torch.full((5, 4), FILL, dtype=torch.int32, device=DEV)              # rows 0 and 4 are guards
    area_a = torch.full((3,), FILL, dtype=torch.int32, device=DEV)
    area_b = torch.full((4,), FILL, dtype=torch.int32, device=DEV)
    for seed in (1, 2):
        a, b = _masks(3, 33, 130, seed), _masks(4, 33, 130, seed + 20)
        assert _raw(torch.from_numpy(a).to(DEV), 3, torch.from_numpy(b).to(DEV), 4, 33, 130, inter[1:4], area_a, area_b) == 0
        want = _reference(a, b)
        assert torch.equal(inter[1:4].cpu().long(), torch.from_numpy(want[0]))
        assert torch.equal(area_a.cpu().long(), torch.from_numpy(want[1])) and torch.equal(area_b.cpu().long(), torch.from_numpy(want[2]))
        assert bool((inter[0] == FILL).all()) and bool((inter[4] == FILL).all())


def test_one_stack():
    from daam_amd.evaluate import mask_overlap_matrix
    a = _masks(11, 63, 65, 9)
    dev_a = torch.from_numpy(a).to(DEV)
    one, two = mask_overlap_matrix(dev_a), mask_overlap_matrix(dev_a, dev_a)
    _assert_exact(one, a)
    for name in ('intersection', 'area_a', 'area_b'):
        assert torch.equal(getattr(one, name), getattr(two, name))
    assert torch.equal(one.intersection, one.intersection.t())
    assert torch.equal(one.intersection.diagonal(), one.area_a) and torch.equal(one.area_a, one.area_b)
    inter = torch.full((11, 11), FILL, dtype=torch.int32, device=DEV)
    area = torch.full((11,), FILL, dtype=torch.int32, device=DEV)
    assert _raw(dev_a, 11, None, 0, 63, 65, inter, area, None) == 0               # area_b = NULL is accepted
    assert torch.equal(inter, one.intersection) and torch.equal(area, one.area_a)


def test_more_than_32_masks():
    from daam_amd.evaluate import mask_overlap_matrix
    a, b = _masks(33, 33, 130, 4), _masks(70, 33, 130, 5)
    _assert_exact(mask_overlap_matrix(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)), a, b)
    c = _masks(40, 33, 130, 6)
    _assert_exact(mask_overlap_matrix(torch.from_numpy(c).to(DEV)), c)


@pytest.mark.parametrize('side', [64, 256])
def test_ratios_equal_the_pair_route(side):
    from daam_amd.evaluate import compute_ioa, compute_iou, mask_overlap_matrix
    a, b = _dense(4, side, side, side), _dense(3, side, side, side + 1, 0.1)
    a[0] = 0                                                                      # an all-zero mask on each side: 0 / 1e-8
    b[0] = 0
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    got = mask_overlap_matrix(ta, tb)
    iou, ioa = got.iou(), got.ioa()
    assert iou.dtype == torch.float32 and ioa.dtype == torch.float32 and iou.shape == (4, 3) and iou.device.type == 'cuda'
    iou, ioa = iou.cpu().numpy(), ioa.cpu().numpy()
    for i in range(4):
        for j in range(3):
            want_iou, want_ioa = compute_iou(ta[i].float(), tb[j].float()), compute_ioa(ta[i].float(), tb[j].float())
            print(f'{side} ({i}, {j}): iou {float(iou[i, j])!r} / {want_iou!r}, ioa {float(ioa[i, j])!r} / {want_ioa!r}')
            assert float(iou[i, j]) == want_iou and float(ioa[i, j]) == want_ioa
    assert iou[0, 0] == 0.0 and ioa[0, 1] == 0.0
    host = got.cpu()
    assert host.intersection.device.type == 'cpu' and np.array_equal(host.iou().numpy(), iou) and np.array_equal(host.ioa().numpy(), ioa)


# ------------------------------------------------------------------------------------------------
# Segmentation
# ------------------------------------------------------------------------------------------------
class _Image:
    def __init__(self, width, height):
        self.size = (width, height)


PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'
WORDS = ['monkey', 'bicycle', 'photo']


def _segmentation():
    from daam_amd import GlobalHeatMap
    from oracle import fake_diffusers as fd
    rng = np.random.default_rng(21)
    maps = torch.from_numpy(np.abs(rng.standard_normal((13, 64, 64))).astype(np.float32)).to(DEV)
    return GlobalHeatMap(fd.FakeTokenizer(), PROMPT, maps).segment(WORDS, _Image(96, 96), threshold=0.3)


def test_segmentation_scores():
    from daam_amd.evaluate import compute_ioa, compute_iou
    seg = _segmentation()
    assert seg.masks.shape == (3, 96, 96) and seg.masks.dtype == torch.uint8 and seg.masks.any()
    host = seg.masks.cpu().numpy()
    own = seg.overlaps()
    _assert_exact(own, host)
    assert seg.ioa_of(WORDS[0], WORDS[1]) == compute_ioa(seg.masks[0].float(), seg.masks[1].float())
    assert torch.equal(seg.ioa(), own.ioa())
    truth = torch.from_numpy(_dense(2, 96, 96, 8)).to(DEV)
    iou = seg.iou(truth).cpu()
    assert iou.shape == (3, 2)
    for i in range(3):
        for j in range(2):
            assert float(iou[i, j]) == compute_iou(seg.masks[i].float(), truth[j].float())
    assert torch.equal(seg.iou(seg), own.iou())                                    # another Segmentation as the truth
    from_host = seg.cpu().overlaps()                                               # CPU masks are moved to the device
    assert from_host.intersection.device.type == 'cuda' and torch.equal(from_host.intersection, own.intersection)
    with pytest.raises(KeyError):
        seg.ioa_of('monkey', 'cat')


# ------------------------------------------------------------------------------------------------
# evaluators
# ------------------------------------------------------------------------------------------------
def test_log_iou_matrix_logs_what_log_iou_logs():
    from daam_amd.evaluate import UnsupervisedEvaluator
    preds = torch.from_numpy(_dense(3, 64, 64, 31)).to(DEV)
    preds[2, :32] = 0
    truths = torch.from_numpy(_dense(2, 64, 64, 32, 0.2)).to(DEV)
    one, many = UnsupervisedEvaluator(), UnsupervisedEvaluator()
    one.log_iou_matrix(preds, truths)
    for g in range(2):
        for p in range(3):
            many.log_iou(preds[p].float(), truths[g].float(), gt_idx=g, pred_idx=p)
    assert list(one.ious) == list(many.ious) == [0, 1]
    assert dict(one.ious) == dict(many.ious)
    assert all(isinstance(v, float) for logged in one.ious.values() for _, v in logged)
    assert one.mean_iou == many.mean_iou and 0.0 < one.mean_iou < 1.0


def test_best_iou_of_byte_candidates():
    from daam_amd.evaluate import MeanEvaluator
    cands = [torch.from_numpy(m).to(DEV) for m in _dense(3, 63, 65, 41)]
    truth = torch.from_numpy(_dense(1, 63, 65, 42, 0.6)[0]).to(DEV)
    bytes_, floats = MeanEvaluator().log_iou(cands, truth), MeanEvaluator().log_iou([c.float() for c in cands], truth.float())
    assert bytes_.ious == floats.ious and 0.0 < bytes_.ious[0] < 1.0
    assert MeanEvaluator().log_iou([c.bool() for c in cands], truth.bool().cpu()).ious == floats.ious


# ------------------------------------------------------------------------------------------------
# the entry point
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,args', [
    ('no masks in a', dict(n_a=0)), ('33 masks in a', dict(n_a=33)), ('33 masks in b', dict(n_b=33)), ('no rows', dict(h=0)),
    ('a is NULL', dict(a=None)), ('inter is NULL', dict(inter=None)), ('b without area_b', dict(area_b=None)),
])
def test_bad_arguments(name, args):
    from daam_amd import _native as nat
    a = torch.ones(33, 5, 13, dtype=torch.uint8, device=DEV)
    b = torch.ones(33, 5, 13, dtype=torch.uint8, device=DEV)
    inter = torch.full((33, 33), FILL, dtype=torch.int32, device=DEV)
    area_a = torch.full((33,), FILL, dtype=torch.int32, device=DEV)
    area_b = torch.full((33,), FILL, dtype=torch.int32, device=DEV)
    call = dict(a=a, n_a=3, b=b, n_b=2, h=5, w=13, inter=inter, area_a=area_a, area_b=area_b)
    call.update(args)
    assert _raw(**call) == nat.E_INVALID, name
    assert nat.load().daam_last_error()
    torch.cuda.synchronize()
    assert bool((inter == FILL).all()) and bool((area_a == FILL).all()) and bool((area_b == FILL).all())


def test_pair_route_is_unaffected():
    from daam_amd.evaluate import mask_overlap, mask_overlap_matrix
    a = torch.from_numpy(_dense(4, 64, 64, 51)).to(DEV)
    b = torch.from_numpy(_dense(4, 64, 64, 52)).to(DEV)
    before = mask_overlap(a.float(), b.float())
    got = mask_overlap_matrix(a, b)
    after = mask_overlap(a.float(), b.float())
    assert torch.equal(before, after)
    assert torch.equal(before[:, 0].to(torch.int32), got.intersection.diagonal())
    assert torch.equal(before[:, 1].to(torch.int32), got.area_a) and torch.equal(before[:, 2].to(torch.int32), got.area_b)
