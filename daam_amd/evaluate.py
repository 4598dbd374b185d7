"""``compute_iou`` / ``compute_ioa`` of the reference's ``daam/evaluate.py:14-35`` on the MI355X: the bicubic resize of the
prediction to the truth mask's size, the binarisation and the three reductions run in one HIP kernel
(``daam_mask_overlap``), for one pair or a whole batch of pairs (the COCO-Gen evaluation loop of ``daam/run/evaluate.py``
calls them once per (word, mask) pair).  Only the final ratio is formed on the host, in fp32 like the reference.

``load_mask`` and the two evaluators of ``daam/evaluate.py:38-117`` (what ``daam/run/evaluate.py`` feeds with these ratios)
are here too: host-side bookkeeping with the reference's names and results; every candidate prediction of one ``log_iou``
call goes to the device in ONE ``daam_mask_overlap`` launch instead of one launch + one host sync per candidate.

``mask_overlap_matrix`` scores two whole STACKS of masks of one size against each other (``daam_mask_overlap_matrix``, DESIGN
3.12): uint8 / bool masks as they are -- e.g. ``Segmentation.masks`` against the truth masks of an image -- every mask byte read
once, exact integer intersections and areas left on the device, and the IoU / IoA matrices formed from them in the reference's
operand order.  It does not resize; the resizing route stays ``mask_overlap``.
"""
from __future__ import annotations

from collections import defaultdict
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as nat

__all__ = ['compute_iou', 'compute_ioa', 'mask_overlap', 'compute_iou_batch', 'compute_ioa_batch', 'load_mask',
           'MeanEvaluator', 'UnsupervisedEvaluator', 'mask_overlap_matrix', 'MaskOverlaps', 'SweepEvaluator', 'mask_boxes',
           'LocalizationEvaluator', 'mask_components', 'MaskComponents', 'image_affinity', 'ImageAffinity']

MAX_MATRIX_MASKS = 32                              # masks per stack of one daam_mask_overlap_matrix call (include/daam_hip.h)


def _to_hip(t: torch.Tensor, name: str, device=None) -> torch.Tensor:
    if t.device.type != 'cuda':
        # the reference's evaluation flow hands over CPU masks (load_mask, and expand_as ends in .cpu()): they are moved
        # to the HIP device (the other operand's, else the current one) -- the arithmetic still runs there and only
        # there, and a box without an MI355X fails right here
        if not torch.cuda.is_available():
            raise RuntimeError(f'daam_amd: {name} is a CPU tensor and no HIP device is visible (there is no CPU fallback)')
        t = t.to(device if device is not None else torch.device('cuda', torch.cuda.current_device()))
    return t


def _as_batch(t: torch.Tensor, name: str, device=None) -> torch.Tensor:
    t = _to_hip(t, name, device)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError(f'{name} must be [h, w] or [n, h, w], got {tuple(t.shape)}')
    return t.to(torch.float32).contiguous()


def mask_overlap(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``a`` [n, ah, aw] (or [ah, aw]) predictions, ``b`` [n, bh, bw] truths -> ``[n, 3]`` fp32 = (sum(a*b), sum(a), sum(b))
    with the reference's preprocessing of ``a``: if ``a.shape[0] != b.shape[0]`` (per pair: the HEIGHTS differ,
    evaluate.py:15) bicubic-resize to ``b``'s size and binarise at 1."""
    dev = a.device if a.device.type == 'cuda' else (b.device if b.device.type == 'cuda' else None)
    a, b = _as_batch(a, 'a', dev), _as_batch(b, 'b', dev)
    if a.shape[0] != b.shape[0]:
        raise ValueError(f'{a.shape[0]} predictions for {b.shape[0]} truth masks')
    if a.device != b.device:
        raise RuntimeError('daam_amd: a and b are on different devices')
    lib = nat.load()
    sums = torch.empty(a.shape[0], 3, dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        nat.check(lib.daam_mask_overlap(a.data_ptr(), a.shape[1], a.shape[2], b.data_ptr(), b.shape[1], b.shape[2], a.shape[0],
                                        sums.data_ptr(), torch.cuda.current_stream(a.device).cuda_stream))
    return sums


def _ratios(sums: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
    s = sums.cpu().numpy().astype(np.float32)
    inter, sa, sb = s[:, 0], s[:, 1], s[:, 2]
    eps = np.float32(1e-8)
    union = sa + sb - inter                                   # evaluate.py:21: a.sum() + b.sum() - intersection (fp32)
    return inter / (union + eps), inter / (sa + eps)


def compute_iou_batch(a: torch.Tensor, b: torch.Tensor) -> np.ndarray:
    return _ratios(mask_overlap(a, b))[0]


def compute_ioa_batch(a: torch.Tensor, b: torch.Tensor) -> np.ndarray:
    return _ratios(mask_overlap(a, b))[1]


def compute_iou(a: torch.Tensor, b: torch.Tensor) -> float:
    """evaluate.py:14-23."""
    return float(compute_iou_batch(a, b)[0])


def compute_ioa(a: torch.Tensor, b: torch.Tensor) -> float:
    """evaluate.py:26-35."""
    return float(compute_ioa_batch(a, b)[0])


@dataclass
class MaskOverlaps:
    """Exact counts of ``mask_overlap_matrix`` (device tensors) and the two ratios of evaluate.py:14-35 formed from them."""
    intersection: torch.Tensor                  # int32 [A, B]: pixels set in a[i] and in b[j]
    area_a: torch.Tensor                        # int32 [A]
    area_b: torch.Tensor                        # int32 [B]

    def iou(self) -> torch.Tensor:
        """f32 [A, B], in fp32 and in ``_ratios``' operand order (evaluate.py:20-23): inter / ((a + b - inter) + 1e-8)."""
        inter = self.intersection.to(torch.float32)
        union = self.area_a.to(torch.float32)[:, None] + self.area_b.to(torch.float32)[None] - inter
        return inter / (union + 1e-8)

    def ioa(self) -> torch.Tensor:
        """f32 [A, B] (evaluate.py:32-35): inter / (a + 1e-8)."""
        return self.intersection.to(torch.float32) / (self.area_a.to(torch.float32)[:, None] + 1e-8)

    def cpu(self) -> 'MaskOverlaps':
        return MaskOverlaps(self.intersection.cpu(), self.area_a.cpu(), self.area_b.cpu())


def _as_masks(t: torch.Tensor, name: str, device=None) -> torch.Tensor:
    """``[n, h, w]`` uint8, contiguous, on the device: uint8 and bool as they are, any other dtype through ``!= 0``."""
    t = _to_hip(t, name, device)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError(f'{name} must be [h, w] or [n, h, w], got {tuple(t.shape)}')
    if t.shape[0] == 0 or t.shape[1] == 0 or t.shape[2] == 0:
        raise ValueError(f'{name} is empty: {tuple(t.shape)}')
    if t.dtype not in (torch.uint8, torch.bool):
        t = t != 0
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _launch_overlap_matrix(a: torch.Tensor, b: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One ``daam_mask_overlap_matrix`` call: ``a`` [A <= 32, h, w], ``b`` [B <= 32, h, w] or None (= ``a``), uint8, contiguous,
    on one device -> (intersection int32 [A, B], area_a int32 [A], area_b int32 [B]).  The counts are below 2^31."""
    n_a, n_b = a.shape[0], (a if b is None else b).shape[0]
    inter = torch.empty(n_a, n_b, dtype=torch.int32, device=a.device)
    area_a = torch.empty(n_a, dtype=torch.int32, device=a.device)
    area_b = area_a if b is None else torch.empty(n_b, dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        nat.check(nat.load().daam_mask_overlap_matrix(
            a.data_ptr(), n_a, None if b is None else b.data_ptr(), n_b, a.shape[1], a.shape[2], inter.data_ptr(), area_a.data_ptr(),
            None if b is None else area_b.data_ptr(), torch.cuda.current_stream(a.device).cuda_stream))
    return inter, area_a, area_b


def mask_overlap_matrix(a: torch.Tensor, b: Optional[torch.Tensor] = None) -> MaskOverlaps:
    """Every mask of ``a`` [A, h, w] (or [h, w]) against every mask of ``b`` [B, h, w] -- ``None``: of ``a`` itself -- in one launch
    per 32 x 32 masks: where both are set, and how many pixels each sets.  uint8 and bool masks go to the kernel as they are (a
    byte != 0 is set), other dtypes through ``!= 0``; CPU tensors are moved to the device.  The masks must have one size: there
    is no resize here (``mask_overlap`` resizes, pair by pair)."""
    dev = a.device if a.device.type == 'cuda' else (b.device if b is not None and b.device.type == 'cuda' else None)
    a = _as_masks(a, 'a', dev)
    if b is not None:
        b = _as_masks(b, 'b', dev)
        if a.shape[1:] != b.shape[1:]:
            raise ValueError(f'masks of {tuple(a.shape[1:])} against masks of {tuple(b.shape[1:])}: mask_overlap_matrix does not resize')
        if a.device != b.device:
            raise RuntimeError('daam_amd: a and b are on different devices')
    step = MAX_MATRIX_MASKS
    cols = a if b is None else b
    if a.shape[0] <= step and cols.shape[0] <= step:
        return MaskOverlaps(*_launch_overlap_matrix(a, b))
    # 32 x 32 blocks, stitched on the device.  With b = None the diagonal blocks are one-stack calls and a block below the
    # diagonal is the transpose of the one above it.
    blocks: Dict[Tuple[int, int], torch.Tensor] = {}
    area_a: Dict[int, torch.Tensor] = {}
    area_b: Dict[int, torch.Tensor] = {}
    for i in range(0, a.shape[0], step):
        for j in range(0, cols.shape[0], step):
            if b is None and j < i:
                blocks[i, j] = blocks[j, i].t()
                continue
            blocks[i, j], area_a[i], area_b[j] = _launch_overlap_matrix(a[i:i + step], None if b is None and i == j else cols[j:j + step])
    inter = torch.cat([torch.cat([blocks[i, j] for j in range(0, cols.shape[0], step)], dim=1) for i in range(0, a.shape[0], step)])
    return MaskOverlaps(inter, torch.cat([area_a[i] for i in sorted(area_a)]), torch.cat([area_b[j] for j in sorted(area_b)]))


def mask_boxes(masks: torch.Tensor) -> torch.Tensor:
    """int32 [M, 4] on the device: the bounding box ``x0 y0 x1 y1`` (inclusive) of the set pixels of every mask of ``masks`` [M, h, w]
    (or [h, w]; uint8 / bool as they are, other dtypes through ``!= 0``; CPU masks are moved to the device), ``(w, h, -1, -1)`` for a
    mask with none: ``daam_localize`` without words, every byte read once, 32 masks per launch."""
    from . import engine
    masks = _as_masks(masks, 'masks')
    step = engine.MAX_LOCATE_TRUTH
    parts = [engine._launch_localize(None, masks.shape[1], masks.shape[2], True, [], masks[i:i + step])[3] for i in range(0, masks.shape[0], step)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


@dataclass
class MaskComponents:
    """The connected components of a stack of masks (``mask_components``): device tensors until ``cpu()`` is asked for.  A component's
    rank is its position when the components of one mask are sorted by their lowest row-major index (``scipy.ndimage.label`` minus
    one)."""
    labels: Optional[torch.Tensor]              # int32 [M, H, W]: the rank of the pixel's component, -1 on background; None if not asked for
    counts: torch.Tensor                        # int32 [M, 2]: components; components of at least min_area pixels
    components: torch.Tensor                    # int32 [M, K, 6]: per rank root, area, x0 y0 x1 y1 (inclusive); (-1, 0, W, H, -1, -1) past the last
    largest: torch.Tensor                       # int32 [M, 6]: the same columns for the largest component (the lowest root on a tie)
    kept: Optional[torch.Tensor]                # uint8 [M, H, W]: the pixels of the components that were kept; None if none were asked for

    def n(self, m: int = 0) -> int:
        """The number of components of mask ``m`` (exact, also beyond the rows of ``components``)."""
        return int(self.counts[m, 0])

    def _listed(self, m: int) -> torch.Tensor:
        return self.components[m, :min(self.n(m), self.components.shape[1])]

    def areas(self, m: int = 0) -> torch.Tensor:
        """int32 [k]: the areas of the listed components of mask ``m``, by rank."""
        return self._listed(m)[:, 1]

    def boxes(self, m: int = 0) -> torch.Tensor:
        """int32 [k, 4]: ``x0 y0 x1 y1`` (inclusive) of the listed components of mask ``m``, by rank."""
        return self._listed(m)[:, 2:6]

    def largest_boxes(self) -> torch.Tensor:
        """int32 [M, 4]: the box of every mask's largest component; ``(W, H, -1, -1)`` for an empty mask, as ``mask_boxes`` gives."""
        return self.largest[:, 2:6]

    def cpu(self) -> 'MaskComponents':
        return MaskComponents(None if self.labels is None else self.labels.cpu(), self.counts.cpu(), self.components.cpu(),
                              self.largest.cpu(), None if self.kept is None else self.kept.cpu())


def mask_components(masks: torch.Tensor, connectivity: int = 8, min_area: int = 0, keep=None, max_components: int = 256,
                    labels: bool = True) -> MaskComponents:
    """``engine.mask_components`` as a ``MaskComponents``: which pixels of every mask of ``masks`` [M, H, W] (or [H, W]) belong
    together -- labels, counts, the list of components, the largest one and, with ``keep`` (``'area'``: at least ``min_area`` pixels,
    ``'largest'``), the cleaned masks -- from one ``daam_mask_components`` call per 32 masks, everything left on the device."""
    from . import engine
    return MaskComponents(*engine.mask_components(masks, connectivity, min_area, keep, max_components, labels))


@dataclass
class ImageAffinity:
    """The propagation weights of one image (``image_affinity``): what ``GlobalHeatMap.refine`` / ``Segmentation.refine`` spread the
    soft maps along.  They depend on the image, the dilations and the scale alone, so one instance serves every word, threshold and
    call on that image (``refine(..., affinity=)``)."""
    weights: torch.Tensor                       # f32 [8 * len(dilations), H, W] on the device (engine.refine_affinity)
    dilations: Tuple[int, ...]
    scale: float
    size: Tuple[int, int]                       # (H, W) of the image

    def refine(self, maps: torch.Tensor, iterations: int = 10, threshold: float = 0.4, masks: bool = True, labels: bool = True):
        """``engine.refine_maps`` of ``maps`` f32 [N, H, W] with these weights: ``(refined, masks or None, labels or None)``."""
        from . import engine
        if tuple(maps.shape[-2:]) != tuple(self.size):
            raise ValueError(f'the affinity is of an image of {self.size[0]} x {self.size[1]}, the maps are {maps.shape[-2]} x {maps.shape[-1]}')
        return engine.refine_maps(self.weights, self.dilations, maps, iterations, threshold, masks, labels)


def image_affinity(image, dilations=(1, 2, 4, 8, 12, 24), scale: float = 0.1) -> ImageAffinity:
    """``engine.refine_affinity`` as an ``ImageAffinity``: ``image`` is a PIL image or a uint8 [H, W], [H, W, 1] or [H, W, 3] array or
    tensor."""
    from . import engine
    weights = engine.refine_affinity(image, dilations, scale)
    return ImageAffinity(weights, tuple(int(d) for d in dilations), float(scale), (int(weights.shape[1]), int(weights.shape[2])))


def load_mask(path: str) -> torch.Tensor:
    """A mask stored the way the reference stores them (``*.gt.png`` / ``*.pred.png``, experiment.py:160-163,218-221): an
    RGBA image whose ALPHA channel is the mask; any non-zero alpha counts (evaluate.py:38-43).  Returns a CPU float tensor
    ``[h, w]`` of 0 / 1 -- file IO; ``compute_iou`` / ``compute_ioa`` move it to the device."""
    import PIL.Image
    rgba = np.asarray(PIL.Image.open(path))
    if rgba.ndim != 3 or rgba.shape[2] < 4:
        raise ValueError(f'{path}: not an RGBA mask image (shape {rgba.shape})')
    return torch.from_numpy(np.ascontiguousarray(rgba[:, :, 3] > 0)).to(torch.float32)


def _best_iou(preds: Union[torch.Tensor, Sequence[torch.Tensor]], truth: torch.Tensor) -> float:
    """max over the candidate predictions of IoU(candidate, truth) (evaluate.py:56,88).  Candidates of one shape are
    stacked and scored in one launch; a ragged list is scored shape group by shape group."""
    if isinstance(preds, torch.Tensor):
        preds = [preds]
    preds = list(preds)
    if not preds:
        raise ValueError('max() arg is an empty sequence')                    # what the reference's max() raises
    if truth.dim() == 2 and all(t.dtype in (torch.uint8, torch.bool) and t.shape == truth.shape for t in [truth] + preds):
        # masks of one size that are bytes already: nothing is resized, the pair route would widen them to f32 and count the
        # same pixels -- one matrix launch on the bytes instead (decided by dtype: looking at the values would synchronise)
        dev = next((t.device for t in [truth] + preds if t.device.type == 'cuda'), None)
        return float(mask_overlap_matrix(torch.stack([_to_hip(p, 'preds', dev) for p in preds]), truth).iou().max())
    groups: Dict[tuple, List[torch.Tensor]] = defaultdict(list)
    for p in preds:
        groups[(tuple(p.shape), p.device)].append(p)
    best = -np.inf
    for members in groups.values():
        stack = torch.stack([m.to(torch.float32) for m in members])
        best = max(best, float(compute_iou_batch(stack, truth.unsqueeze(0).expand(len(members), -1, -1)).max()))
    return best


class UnsupervisedEvaluator:
    """evaluate.py:46-82: IoUs logged per (ground-truth segment, predicted segment); ``mean_iou`` matches predicted to
    ground-truth indices with the Hungarian algorithm on the summed-IoU matrix and averages over the matched cells."""

    def __init__(self, name: str = 'UnsupervisedEvaluator'):
        self.name = name
        self.ious = defaultdict(list)
        self.num_samples = 0

    def log_iou(self, preds, truth: torch.Tensor, gt_idx: int = 0, pred_idx: int = 0):
        self.ious[gt_idx].append((pred_idx, _best_iou(preds, truth)))

    def log_iou_matrix(self, preds: torch.Tensor, truths: torch.Tensor):
        """What ``log_iou(preds[p], truths[g], gt_idx=g, pred_idx=p)`` logs for every ``g`` and, under it, every ``p`` -- in that
        order -- from one ``mask_overlap_matrix`` launch and one copy to the host.  ``preds`` [P, h, w] and ``truths`` [G, h, w]
        are masks of one size (a value != 0 is set)."""
        iou = mask_overlap_matrix(preds, truths).iou().cpu().numpy()
        for g in range(iou.shape[1]):
            for p in range(iou.shape[0]):
                self.ious[g].append((p, float(iou[p, g])))

    @property
    def mean_iou(self) -> float:
        from scipy.optimize import linear_sum_assignment
        entries = [(g, p, v) for g, logged in self.ious.items() for p, v in logged]
        n = max(max(g, p) for g, p, _ in entries) + 1
        total, count = np.zeros((n, n)), np.zeros((n, n))
        for g, p, v in entries:
            total[g, p] += v
            count[g, p] += 1
        rows, cols = linear_sum_assignment(total, maximize=True)
        return total[rows, cols].sum() / count[rows, cols].sum()

    def increment(self):
        self.num_samples += 1

    def __len__(self) -> int:
        return self.num_samples

    def __str__(self):
        return f'{self.name}<{self.mean_iou:.4f} (mIoU) {len(self)} samples>'


class MeanEvaluator:
    """evaluate.py:85-117: running lists of best-candidate IoUs and of mean heat intensities, their means and the
    1.96-sigma half width of the mean IoU."""

    def __init__(self, name: str = 'MeanEvaluator'):
        self.ious: List[float] = []
        self.intensities: List[float] = []
        self.name = name

    def log_iou(self, preds, truth: torch.Tensor) -> 'MeanEvaluator':
        self.ious.append(_best_iou(preds, truth))
        return self

    def log_intensity(self, pred: torch.Tensor) -> 'MeanEvaluator':
        self.intensities.append(pred.mean().item())
        return self

    @property
    def mean_iou(self) -> float:
        return np.mean(self.ious)

    @property
    def mean_intensity(self) -> float:
        return np.mean(self.intensities)

    @property
    def ci95_miou(self) -> float:
        return 1.96 * np.std(self.ious) / np.sqrt(len(self.ious))

    def __len__(self) -> int:
        return max(len(self.ious), len(self.intensities))

    def __str__(self):
        return (f'{self.name}<{self.mean_iou:.4f} (±{self.ci95_miou:.3f} mIoU) {self.mean_intensity:.4f} (mInt) '
                f'{len(self)} samples>')


class SweepEvaluator:
    """``MeanEvaluator``'s mean IoU as a curve over the threshold: ``log`` takes the ``heatmap.ThresholdSweep`` of one image and
    appends, per threshold, what ``MeanEvaluator.log_iou`` would log there -- the best IoU among the candidate pairings of a word --
    so one pass over a data set gives the mIoU at every threshold and the threshold to report."""

    def __init__(self, name: str = 'SweepEvaluator'):
        self.name = name
        self.thresholds: Optional[np.ndarray] = None       # f32 [T], set by the first log
        self.ious: List[np.ndarray] = []                   # one f32 [T] per logged word

    def log(self, sweep, pairs: Optional[Sequence[Tuple[int, int]]] = None) -> 'SweepEvaluator':
        """``pairs=None``: one entry per word of ``sweep``, its IoU with the truth mask it matches best (per threshold).
        ``pairs``: one entry per ``(word index, truth index)``.  One copy to the host per call."""
        thr = sweep.thresholds.cpu().numpy().astype(np.float32)
        if self.thresholds is None:
            self.thresholds = thr
        elif thr.shape != self.thresholds.shape or not (thr == self.thresholds).all():
            raise ValueError('SweepEvaluator: this sweep has other thresholds than the ones logged so far')
        iou = sweep.iou()
        if iou.shape[1] == 0:
            raise ValueError('SweepEvaluator: the sweep has no truth masks')
        rows = iou.max(dim=1).values if pairs is None else torch.stack([iou[int(w), int(g)] for w, g in pairs])
        self.ious.extend(rows.cpu().numpy().astype(np.float32))
        return self

    @property
    def mean_iou(self) -> np.ndarray:
        """f32 [T]: per threshold, ``MeanEvaluator.mean_iou`` of the values logged there."""
        cols = np.ascontiguousarray(np.stack(self.ious).astype(np.float64).T)
        return np.array([np.mean(c) for c in cols], dtype=np.float32)

    @property
    def best(self) -> Tuple[float, float]:
        """``(threshold, mIoU)`` of the largest mean IoU; the lowest such threshold on a tie."""
        curve = self.mean_iou
        t = min(np.flatnonzero(curve == curve.max()), key=lambda i: self.thresholds[i])
        return float(self.thresholds[t]), float(curve[t])

    def __len__(self) -> int:
        return len(self.ious)

    def __str__(self):
        thr, miou = self.best
        return f'{self.name}<{miou:.4f} (mIoU) at threshold {thr:g}, {len(self.thresholds)} thresholds, {len(self)} samples>'


class LocalizationEvaluator:
    """The two localisation measures over a data set, modelled on ``SweepEvaluator``: ``log`` takes the ``heatmap.Localization`` of
    one image and appends, per word, whether its peak hits a truth mask (the pointing game) and, per threshold, its box IoU with a
    truth box; ``pointing_accuracy`` is the share of hits and ``corloc`` the share of entries whose box IoU is at least 0.5."""
    IOU_BAR = 0.5

    def __init__(self, name: str = 'LocalizationEvaluator'):
        self.name = name
        self.thresholds: Optional[np.ndarray] = None       # f32 [T], set by the first log
        self.hits: List[bool] = []                         # one per logged entry
        self.ious: List[np.ndarray] = []                   # one f32 [T] per logged entry

    def log(self, loc, pairs: Optional[Sequence[Tuple[int, int]]] = None) -> 'LocalizationEvaluator':
        """``pairs=None``: one entry per word of ``loc``, judged against the truth mask that serves it best (a hit in any mask; per
        threshold the largest box IoU).  ``pairs``: one entry per ``(word index, truth index)``.  One copy to the host per call."""
        thr = loc.thresholds.cpu().numpy().astype(np.float32)
        if self.thresholds is None:
            self.thresholds = thr
        elif thr.shape != self.thresholds.shape or not (thr == self.thresholds).all():
            raise ValueError('LocalizationEvaluator: this localization has other thresholds than the ones logged so far')
        if loc.hits is None or loc.hits.shape[1] == 0:
            raise ValueError('LocalizationEvaluator: the localization has no truth masks')
        iou, hits = loc.box_iou().cpu().numpy().astype(np.float32), loc.hits.cpu().numpy().astype(bool)
        if pairs is None:
            self.hits.extend(bool(h) for h in hits.any(1))
            self.ious.extend(iou.max(1))
        else:
            self.hits.extend(bool(hits[int(w), int(g)]) for w, g in pairs)
            self.ious.extend(iou[int(w), int(g)] for w, g in pairs)
        return self

    @property
    def pointing_accuracy(self) -> float:
        return float(np.mean(self.hits))

    @property
    def corloc(self) -> np.ndarray:
        """f32 [T]: per threshold, the share of the logged entries whose box IoU is >= 0.5."""
        return (np.stack(self.ious) >= np.float32(self.IOU_BAR)).mean(0).astype(np.float32)

    @property
    def best(self) -> Tuple[float, float]:
        """``(threshold, CorLoc)`` of the largest CorLoc; the lowest such threshold on a tie."""
        curve = self.corloc
        t = min(np.flatnonzero(curve == curve.max()), key=lambda i: self.thresholds[i])
        return float(self.thresholds[t]), float(curve[t])

    def __len__(self) -> int:
        return len(self.hits)

    def __str__(self):
        thr, best = self.best
        return (f'{self.name}<{self.pointing_accuracy:.4f} (pointing) {best:.4f} (CorLoc) at threshold {thr:g}, '
                f'{len(self.thresholds)} thresholds, {len(self)} samples>')
