"""Heat-map containers with the reference's names (``daam/heatmap.py``): the raw
per-(factor, layer, head) collection -- here a zero-copy view over the device running sums --
and ``GlobalHeatMap`` / ``WordHeatMap``, whose arithmetic runs in ``libdaam_hip.so``."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import Any, ClassVar, Iterable, Iterator, List, Optional, Sequence, Set, Tuple, Union

import torch

from . import engine as _engine
from .utils import cached_nlp, compute_token_merge_indices

__all__ = ['GlobalHeatMap', 'RawHeatMapCollection', 'WordHeatMap', 'ParsedHeatMap', 'SyntacticHeatMapPair', 'Segmentation',
           'RegionAttribution', 'KeyScores', 'ThresholdSweep', 'Localization', 'SelfAffinity', 'Discovery']

RawHeatMapKey = Tuple[int, int, int]  # factor, layer, head


class RawHeatMapCollection:
    """Same surface as reference heatmap.py:148-172 (``update / factors / layers / heads /
    __iter__ / clear``).  Iteration yields ``((factor, layer, head), Tensor[tokens, h, w])`` in
    first-update order; the tensors are views of the live device buffers."""

    def __init__(self, engine: '_engine.HeatMapEngine'):
        self._engine = engine

    def update(self, factor: int, layer_idx: int, head_idx: int, heatmap: torch.Tensor):
        self._engine.add_map(factor, layer_idx, head_idx, heatmap)

    def factors(self) -> Set[int]:
        return {k[0] for k in self._engine.keys()}

    def layers(self) -> Set[int]:
        return {k[1] for k in self._engine.keys()}

    def heads(self) -> Set[int]:
        return {k[2] for k in self._engine.keys()}

    def __iter__(self) -> Iterator[Tuple[RawHeatMapKey, torch.Tensor]]:
        if self._engine.time_bins is not None:
            raise RuntimeError('this trace has time_bins: it keeps one sum per window, use raw_heat_maps(time_bin)')
        return self._engine.items()

    def __len__(self) -> int:
        return len(self._engine.keys())

    def clear(self):
        self._engine.clear()


class WordHeatMap:
    """reference heatmap.py:56-96."""

    def __init__(self, heatmap: torch.Tensor, word: Optional[str] = None, word_idx: Optional[int] = None):
        self.word = word
        self.word_idx = word_idx
        self.heatmap = heatmap

    @property
    def value(self) -> torch.Tensor:
        return self.heatmap

    def expand_as(self, image, absolute: bool = False, threshold: Optional[float] = None, plot: bool = False,
                  **plot_kwargs) -> torch.Tensor:
        """Bicubic to ``(image.size[0], image.size[1])`` (PIL order, as the reference passes
        it, heatmap.py:80), min-max normalise unless ``absolute``, optional threshold; returns a
        CPU tensor like the reference (heatmap.py:88).  A word map of unequal sides (a non-square generation,
        ``trace(pipe, height=, width=)``) is resized to ``(image.size[1], image.size[0])`` = ``[image height, image width]`` instead:
        PIL's ``size`` is (width, height), which the reference's order only survives on square images."""
        size = (image.size[0], image.size[1]) if self.heatmap.shape[-2] == self.heatmap.shape[-1] else (image.size[1], image.size[0])
        out = _engine.expand_word_map(self.heatmap.float(), int(size[0]), int(size[1]),
                                      absolute=absolute, threshold=threshold)
        out = out.cpu()
        if plot:
            self.plot_overlay(image, **plot_kwargs)
        return out

    def compute_ioa(self, other: 'WordHeatMap') -> float:
        """reference heatmap.py:95-96."""
        from .evaluate import compute_ioa
        return compute_ioa(self.heatmap, other.heatmap)

    def plot_overlay(self, image, out_file=None, color_normalize=True, ax=None, **expand_kwargs):
        from .plotting import plot_overlay_heat_map
        plot_overlay_heat_map(image, self.expand_as(image, **expand_kwargs), word=self.word, out_file=out_file,
                              color_normalize=color_normalize, ax=ax)


@dataclass
class SyntacticHeatMapPair:
    """A dependency arc of the prompt with the word maps at both ends (heatmap.py:99-105)."""
    head_heat_map: WordHeatMap
    dep_heat_map: WordHeatMap
    head_text: str
    dep_text: str
    relation: str


@dataclass
class ParsedHeatMap:
    """A parsed prompt token with its word map (heatmap.py:108-111); ``token`` is the parser's token object."""
    word_heat_map: WordHeatMap
    token: Any


@dataclass
class Segmentation:
    """Masks of several words of one prompt at image resolution and the map of which word owns each pixel
    (``GlobalHeatMap.segment``).  Everything lives on the device until ``cpu()`` is asked for."""
    BACKGROUND: ClassVar[int] = 255             # label of a pixel where no word exceeds the threshold

    words: List[str]
    word_heat_maps: List[WordHeatMap]
    masks: torch.Tensor                         # uint8 [len(words), height, width]: 1 where the word's expanded map > threshold
    labels: Optional[torch.Tensor]              # uint8 [height, width]: index into ``words`` or BACKGROUND; None if not computed
    refined: Optional[torch.Tensor] = None      # f32 [len(words), height, width]: the refined soft maps behind ``masks`` (``refine``); else None

    def mask(self, word: str) -> torch.Tensor:
        """The uint8 [height, width] mask of ``word`` (its first entry, when the word was asked for twice)."""
        if word not in self.words:
            raise KeyError(word)
        return self.masks[self.words.index(word)]

    def overlaps(self, truth: Union[None, torch.Tensor, 'Segmentation'] = None):
        """``evaluate.MaskOverlaps`` of the word masks against ``truth`` (a stack of masks of this size, or another
        ``Segmentation``; ``None``: the words against each other): exact intersections and areas from one launch on the bytes
        (``evaluate.mask_overlap_matrix``); CPU masks are moved to the device."""
        from .evaluate import mask_overlap_matrix
        return mask_overlap_matrix(self.masks, truth.masks if isinstance(truth, Segmentation) else truth)

    def iou(self, truth: Union[torch.Tensor, 'Segmentation']) -> torch.Tensor:
        """f32 [len(words), len(truth)]: ``compute_iou`` (evaluate.py:14-23) of every word mask with every truth mask."""
        return self.overlaps(truth).iou()

    def ioa(self, truth: Union[None, torch.Tensor, 'Segmentation'] = None) -> torch.Tensor:
        """f32 [len(words), ...]: ``compute_ioa`` (evaluate.py:26-35); ``None``: of every word's mask with every other word's."""
        return self.overlaps(truth).ioa()

    def ioa_of(self, word_a: str, word_b: str) -> float:
        """``WordHeatMap.compute_ioa`` (heatmap.py:95-96) of the thresholded masks of two words: |a and b| / |a|."""
        from .evaluate import mask_overlap_matrix
        return float(mask_overlap_matrix(self.mask(word_a), self.mask(word_b)).ioa()[0, 0])

    def components(self, connectivity: int = 8, min_area: int = 0):
        """``evaluate.MaskComponents`` of the word masks: per word the labelled blobs, their number, areas and boxes and the largest
        one (``evaluate.mask_components``)."""
        from .evaluate import mask_components
        return mask_components(self.masks, connectivity=connectivity, min_area=min_area)

    def clean(self, min_area: int = 0, largest: bool = False, connectivity: int = 8) -> 'Segmentation':
        """A ``Segmentation`` of the same words and word heat maps whose masks keep only the blobs of at least ``min_area`` pixels
        or, with ``largest``, every word's largest blob alone (and nothing when that has fewer than ``min_area`` pixels); it has no
        label map.  ``iou`` / ``ioa`` / ``attribute`` run on the cleaned masks as on any others."""
        from . import engine
        _, _, _, big, kept = engine.mask_components(self.masks, connectivity, 0 if largest else min_area, 'largest' if largest else 'area',
                                                    max_components=0, labels=False)
        if largest and min_area > 0:
            kept = kept * (big[:, 1] >= int(min_area)).to(torch.uint8)[:, None, None]
        return Segmentation(list(self.words), list(self.word_heat_maps), kept, None)

    def refine(self, image, threshold: float = 0.4, iterations: int = 10, dilations=_engine.REFINE_DILATIONS, scale: float = 0.1,
               absolute: bool = False, labels: bool = True, affinity=None) -> 'Segmentation':
        """``GlobalHeatMap.refine`` of the same words, starting from ``word_heat_maps``: the expanded soft maps are propagated along
        ``image``'s local colour affinities and thresholded again."""
        return _refine_words(list(self.words), list(self.word_heat_maps), image, threshold, iterations, dilations, scale, absolute, labels,
                             affinity)

    def cpu(self) -> 'Segmentation':
        maps = [WordHeatMap(m.heatmap.cpu(), m.word, m.word_idx) for m in self.word_heat_maps]
        return Segmentation(list(self.words), maps, self.masks.cpu(), None if self.labels is None else self.labels.cpu(),
                            None if self.refined is None else self.refined.cpu())


def _refine_words(words: List[str], heat: List[WordHeatMap], image, threshold: float, iterations: int, dilations, scale: float,
                  absolute: bool, labels: bool, affinity) -> Segmentation:
    """What ``GlobalHeatMap.refine`` and ``Segmentation.refine`` share: every word map expanded as ``expand_as(image, absolute=)``
    expands it (on the device), ``iterations`` rounds of ``engine.refine_maps`` along the image's affinities, masks and labels."""
    from .evaluate import ImageAffinity, image_affinity
    if not heat:
        raise ValueError('refine needs at least one word')
    if labels and len(heat) > _engine.MAX_REFINE_MAPS:
        raise ValueError(f'a label map orders at most {_engine.MAX_REFINE_MAPS} words, got {len(heat)}; pass labels=False for masks only')
    plane = heat[0].heatmap
    pil = (image.shape[1], image.shape[0]) if hasattr(image, 'shape') else image.size       # an array's (width, height), PIL's size
    size = (pil[0], pil[1]) if plane.shape[-2] == plane.shape[-1] else (pil[1], pil[0])
    if affinity is None:
        affinity = image_affinity(image, dilations, scale)
    elif not isinstance(affinity, ImageAffinity):
        raise TypeError(f'affinity must be an ImageAffinity (daam_amd.image_affinity), got {type(affinity).__name__}')
    if tuple(affinity.size) != (int(size[0]), int(size[1])):
        raise ValueError(f'the affinity is of an image of {affinity.size[0]} x {affinity.size[1]}, the expanded maps are '
                         f'{int(size[0])} x {int(size[1])}')
    soft = torch.stack([_engine.expand_word_map(m.heatmap.float(), int(size[0]), int(size[1]), absolute=absolute) for m in heat])
    refined, masks, label_map = affinity.refine(soft, iterations, threshold, True, labels)
    return Segmentation(words, heat, masks, label_map, refined)


@dataclass
class ThresholdSweep:
    """The pixel counts behind IoU / IoA of every word's mask against every truth mask at every threshold
    (``GlobalHeatMap.threshold_sweep``): what ``segment(threshold=t)`` followed by ``Segmentation.overlaps(truth)`` counts, for all
    ``t`` from two passes at image resolution.  Everything lives on the device until ``cpu()`` is asked for."""
    words: List[str]
    thresholds: torch.Tensor                    # f32 [T], in the caller's order
    intersection: torch.Tensor                  # int32 [W, G, T]: pixels where word w's value > thresholds[t] and truth g is set
    area_pred: torch.Tensor                     # int32 [W, T]: pixels where word w's value > thresholds[t]
    area_truth: torch.Tensor                    # int32 [G]

    def iou(self) -> torch.Tensor:
        """f32 [W, G, T], in ``evaluate._ratios``' operand order: inter / ((pred + truth - inter) + 1e-8) -- ``[..., t]`` is
        bit-equal to ``Segmentation.iou`` at ``thresholds[t]``."""
        inter = self.intersection.to(torch.float32)
        union = self.area_pred.to(torch.float32)[:, None, :] + self.area_truth.to(torch.float32)[None, :, None] - inter
        return inter / (union + 1e-8)

    def ioa(self) -> torch.Tensor:
        """f32 [W, G, T]: inter / (pred + 1e-8), ``Segmentation.ioa`` at every threshold."""
        return self.intersection.to(torch.float32) / (self.area_pred.to(torch.float32)[:, None, :] + 1e-8)

    def precision(self) -> torch.Tensor:
        return self.ioa()

    def recall(self) -> torch.Tensor:
        """f32 [W, G, T]: inter / (truth + 1e-8)."""
        return self.intersection.to(torch.float32) / (self.area_truth.to(torch.float32)[None, :, None] + 1e-8)

    def _word(self, word: Union[str, int]) -> int:
        if isinstance(word, str):
            if word not in self.words:
                raise KeyError(word)
            return self.words.index(word)
        return int(word)

    def best(self, word: Union[str, int], truth_idx: int = 0) -> Tuple[float, float]:
        """``(threshold, iou)`` of the largest IoU of ``word`` (a word of ``words`` or its index) against truth mask
        ``truth_idx``; the lowest such threshold on a tie."""
        curve = self.iou()[self._word(word), truth_idx].cpu()
        best = curve.max()
        thr = self.thresholds.cpu()
        t = min(range(len(curve)), key=lambda i: (not bool(curve[i] == best), float(thr[i])))
        return float(thr[t]), float(curve[t])

    def mean_best_iou(self) -> torch.Tensor:
        """f32 [T]: the mean over the words of each word's best IoU over the truth masks -- per threshold, what
        ``MeanEvaluator.log_iou`` logs (the best candidate pairing), averaged."""
        return self.iou().max(dim=1).values.mean(dim=0)

    def best_threshold(self) -> float:
        """The threshold with the largest ``mean_best_iou()``; the lowest such on a tie."""
        curve, thr = self.mean_best_iou().cpu(), self.thresholds.cpu()
        best = curve.max()
        return float(min((float(thr[i]) for i in range(len(curve)) if bool(curve[i] == best))))

    def at(self, threshold: float):
        """``evaluate.MaskOverlaps`` of one threshold of the sweep (KeyError when it was not swept)."""
        from .evaluate import MaskOverlaps
        hits = (self.thresholds.cpu() == torch.tensor(threshold, dtype=torch.float32)).nonzero()
        if not len(hits):
            raise KeyError(threshold)
        t = int(hits[0])
        return MaskOverlaps(self.intersection[:, :, t], self.area_pred[:, t], self.area_truth)

    def cpu(self) -> 'ThresholdSweep':
        return ThresholdSweep(list(self.words), self.thresholds.cpu(), self.intersection.cpu(), self.area_pred.cpu(), self.area_truth.cpu())


def _box_iou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """IoU of inclusive pixel boxes ``a`` [..., 4] and ``b`` [..., 4] (broadcast), f32; an empty box (x1 < x0) scores 0.  The areas
    are exact in int64 and the ratio is formed in float64 and rounded once."""
    a, b = a.to(torch.int64), b.to(torch.int64)
    area_a = (a[..., 2] - a[..., 0] + 1).clamp(min=0) * (a[..., 3] - a[..., 1] + 1).clamp(min=0)
    area_b = (b[..., 2] - b[..., 0] + 1).clamp(min=0) * (b[..., 3] - b[..., 1] + 1).clamp(min=0)
    iw = (torch.minimum(a[..., 2], b[..., 2]) - torch.maximum(a[..., 0], b[..., 0]) + 1).clamp(min=0)
    ih = (torch.minimum(a[..., 3], b[..., 3]) - torch.maximum(a[..., 1], b[..., 1]) + 1).clamp(min=0)
    inter = torch.where((area_a > 0) & (area_b > 0), iw * ih, torch.zeros_like(iw))
    union = area_a + area_b - inter
    return (inter.to(torch.float64) / union.clamp(min=1).to(torch.float64)).to(torch.float32)


@dataclass
class Localization:
    """Where the words of one prompt lie in an image (``GlobalHeatMap.localize``): the bounding box of every word's mask at every
    threshold, the peak of every word's expanded map, the boxes of the truth masks and whether each peak lies inside each truth
    mask (the pointing game) -- from one pass at image resolution.  Everything lives on the device until ``cpu()`` is asked for."""
    words: List[str]
    thresholds: torch.Tensor                    # f32 [T], in the caller's order
    size: Tuple[int, int]                       # (height, width) of the output
    boxes: torch.Tensor                         # int32 [W, T, 4]: x0 y0 x1 y1, inclusive; (width, height, -1, -1) when empty
    peaks: torch.Tensor                         # int32 [W, 2]: x, y
    peak_values: torch.Tensor                   # f32 [W, 3]: the raw expanded value at the peak, the minimum, the maximum
    truth_boxes: Optional[torch.Tensor]         # int32 [G, 4], or None without truth masks
    hits: Optional[torch.Tensor]                # bool [W, G]: the peak of word w lies in truth mask g; None without truth masks

    def _word(self, word: Union[str, int]) -> int:
        if isinstance(word, str):
            if word not in self.words:
                raise KeyError(word)
            return self.words.index(word)
        return int(word)

    def box(self, word: Union[str, int], threshold: Optional[float] = None) -> Optional[Tuple[int, int, int, int]]:
        """``(x0, y0, x1, y1)`` of ``word`` at ``threshold`` (``None``: the first one), ``None`` when its mask is empty there;
        KeyError for a threshold that was not asked for."""
        t = 0
        if threshold is not None:
            found = (self.thresholds.cpu() == torch.tensor(threshold, dtype=torch.float32)).nonzero()
            if not len(found):
                raise KeyError(threshold)
            t = int(found[0])
        x0, y0, x1, y1 = (int(v) for v in self.boxes[self._word(word), t].cpu())
        return None if x1 < x0 else (x0, y0, x1, y1)

    def box_iou(self, truth_boxes: Optional[torch.Tensor] = None) -> torch.Tensor:
        """f32 [W, G, T]: the IoU of every word's box at every threshold with every box of ``truth_boxes`` [G, 4] (inclusive pixel
        boxes; default: the boxes of the truth masks); an empty box scores 0."""
        truth_boxes = self.truth_boxes if truth_boxes is None else torch.as_tensor(truth_boxes).reshape(-1, 4).to(self.boxes.device)
        if truth_boxes is None:
            raise ValueError('box_iou needs truth boxes: the localization has no truth masks')
        return _box_iou(self.boxes[:, None, :, :], truth_boxes[None, :, None, :])

    def pointing(self) -> torch.Tensor:
        """bool [W, G]: the pointing game -- the peak of word w lies inside truth mask g."""
        if self.hits is None:
            raise ValueError('pointing needs truth masks')
        return self.hits

    def cpu(self) -> 'Localization':
        return Localization(list(self.words), self.thresholds.cpu(), self.size, self.boxes.cpu(), self.peaks.cpu(), self.peak_values.cpu(),
                            None if self.truth_boxes is None else self.truth_boxes.cpu(), None if self.hits is None else self.hits.cpu())


@dataclass
class RegionAttribution:
    """Which prompt tokens put their attention inside each of M image regions (``GlobalHeatMap.attribute``): the sums of every
    token row's expanded heat map (``expand_as(absolute=True)``, no min-max, no threshold) under each region's mask.  Everything
    lives on the device until ``cpu()`` is asked for."""
    scores: torch.Tensor                        # f32 [M, rows]: sum over the region's pixels of row t's expanded map
    area: torch.Tensor                          # int32 [M]: pixels of each region
    footprint: torch.Tensor                     # f32 [M, h, w]: the masks pulled back onto the maps' grid (``engine.region_dots``)
    tokenizer: Any = None
    prompt: Optional[str] = None

    def mean(self) -> torch.Tensor:
        """f32 [M, rows]: the mean expanded value inside each region, ``scores / max(area, 1)``."""
        return self.scores / self.area.clamp(min=1).to(torch.float32)[:, None]

    def word_scores(self, words: Sequence[Union[str, Tuple[str, Optional[int]]]]) -> torch.Tensor:
        """f32 [M, len(words)]: the mean of ``scores`` over each word's token rows (``compute_token_merge_indices``) -- by
        linearity the score of ``compute_word_heat_map(word)`` under each region."""
        cols = []
        for word in words:
            w, i = (word, None) if isinstance(word, str) else (word[0], word[1])
            idxs, _ = compute_token_merge_indices(self.tokenizer, self.prompt, w, i)
            cols.append(self.scores[:, list(idxs)].mean(dim=1))
        return torch.stack(cols, dim=1)

    def top_words(self, words: Sequence[Union[str, Tuple[str, Optional[int]]]], k: int = 1):
        """``torch.topk`` of ``word_scores(words)`` along the words: ``(values, indices)``, each [M, k]."""
        return torch.topk(self.word_scores(words), k, dim=1)

    def cpu(self) -> 'RegionAttribution':
        return RegionAttribution(self.scores.cpu(), self.area.cpu(), self.footprint.cpu(), self.tokenizer, self.prompt)


@dataclass
class KeyAnalysis:
    """What the per-key results (``KeyScores``, ``KeyCoattention``) share: the keys of the selection and what names and crops them.
    The subclasses write their own ``__init__`` to keep their tensors second among the positional arguments."""
    keys: List[RawHeatMapKey]                   # (factor, layer, head), in the library's key order
    layer_names: Optional[List[str]] = None     # the trace's layer names, indexed by a key's layer
    tokenizer: Any = None
    prompt: Optional[str] = None

    def index_of(self, key) -> int:
        """The position of ``key`` in ``keys``: ``(factor, layer, head)`` with the layer as an index or as a name of
        ``layer_names``, or a ``(key, score)`` pair as ``top_keys`` returns them.  ValueError for a key the selection lacks."""
        if len(key) == 2 and isinstance(key[0], (tuple, list)):
            key = key[0]
        factor, layer, head = key
        if isinstance(layer, str):
            if self.layer_names is None or layer not in self.layer_names:
                raise ValueError(f'key {tuple(key)!r}: no layer of that name')
            # the reference's names restart per block, so the factor and the head help to tell the layers apart
            found = [i for i, name in enumerate(self.layer_names) if name == layer and (int(factor), i, int(head)) in self.keys]
            if len(found) > 1:
                raise ValueError(f'key {tuple(key)!r}: layers {found} share that name and factor; pass the layer\'s index')
            layer = found[0] if found else -1
        try:
            return self.keys.index((int(factor), int(layer), int(head)))
        except ValueError:
            raise ValueError(f'key {tuple(key)!r} is not among the {len(self.keys)} keys of the selection') from None

    def _grouped(self, pos: int, values: torch.Tensor):
        """``(labels, means)``: ``values`` [K, ...] averaged over the keys that share element ``pos`` of their key, labels ascending."""
        labels = sorted({key[pos] for key in self.keys})
        rows = [values[[i for i, key in enumerate(self.keys) if key[pos] == label]].mean(dim=0) for label in labels]
        return labels, torch.stack(rows)


@dataclass(init=False)
class KeyScores(KeyAnalysis):
    """Head analysis (``DiffusionHeatMapHooker.compute_key_scores``): for every selected ``(factor, layer, head)`` key what
    ``compute_global_heat_map(head_idx=, layer_idx=)`` + ``attribute(regions)`` would give for that key alone -- the sum of every token
    row's clamped, resized map under each region -- from one pass over the running sums.  On the device until ``cpu()``."""
    scores: torch.Tensor                        # f32 [K, M, rows]; M = 1 without regions (the total clamped mass)
    area: Optional[torch.Tensor]                # int32 [M] pixels of each region; None without masks at image resolution

    def __init__(self, keys, scores, area, layer_names=None, tokenizer=None, prompt=None):
        super().__init__(keys, layer_names, tokenizer, prompt)
        self.scores, self.area = scores, area

    def mean(self) -> torch.Tensor:
        """f32 [M, rows]: the mean over the keys -- by linearity ``GlobalHeatMap.attribute(regions).scores`` of the same selection."""
        return self.scores.mean(dim=0)

    def word_scores(self, word: str, word_idx: Optional[int] = None) -> torch.Tensor:
        """f32 [K, M]: the mean over the word's token rows (the merge indices of ``compute_word_heat_map``)."""
        idxs, _ = compute_token_merge_indices(self.tokenizer, self.prompt, word, word_idx)
        return self.scores[:, :, list(idxs)].mean(dim=2)

    def top_keys(self, word: str, region: int = 0, k: int = 10, word_idx: Optional[int] = None):
        """The ``k`` keys that put most of ``word`` into ``region``: ``[((factor, layer, head), score)]``, highest first; equal
        scores keep the key order."""
        col = self.word_scores(word, word_idx)[:, region].cpu()
        order = torch.sort(col, descending=True, stable=True).indices[:k].tolist()
        return [(self.keys[i], float(col[i])) for i in order]

    def by_layer(self):
        """``(layers, f32 [len(layers), M, rows])``: the mean over each layer's heads, layers ascending."""
        return self._grouped(1, self.scores)

    def by_head(self):
        """``(heads, f32 [len(heads), M, rows])``: the mean over the layers that have the head, heads ascending."""
        return self._grouped(2, self.scores)

    def cpu(self) -> 'KeyScores':
        return KeyScores(list(self.keys), self.scores.cpu(), None if self.area is None else self.area.cpu(), self.layer_names,
                         self.tokenizer, self.prompt)


class SelfAffinity:
    """The self-attention affinity of a traced generation (``trace(pipe, self_affinity=True)`` -> ``compute_self_affinity()``;
    DESIGN 3.22): ``sums`` f32 [P, P], P = h w cells of ``grid``, is the sum over every tapped ``attn1`` call and head of
    ``softmax(Q K^T scale)`` -- ``slices`` row-stochastic matrices from ``calls`` calls, so every row sums to ``slices``."""

    def __init__(self, sums: torch.Tensor, grid: Tuple[int, int], slices: int, calls: int):
        grid = (int(grid[0]), int(grid[1]))
        if sums.dim() != 2 or sums.shape[0] != sums.shape[1] or sums.shape[0] != grid[0] * grid[1]:
            raise ValueError(f'sums {tuple(sums.shape)} are not the [P, P] matrix of a grid of {grid[0]} x {grid[1]} cells')
        self.sums, self.grid, self.slices, self.calls = sums, grid, int(slices), int(calls)

    def matrix(self) -> torch.Tensor:
        """f32 [P, P]: ``sums`` with every row divided by its sum (a row of zeros stays zero)."""
        total = self.sums.sum(dim=1, keepdim=True)
        return self.sums / torch.where(total == 0, torch.ones_like(total), total)

    def of(self, y: int, x: int) -> torch.Tensor:
        """f32 [h, w]: the affinity of the cell ``(y, x)`` to every cell, its row of ``matrix()``."""
        h, w = self.grid
        if not (0 <= y < h and 0 <= x < w):
            raise ValueError(f'cell ({y}, {x}) is outside the grid of {h} x {w}')
        row = self.sums[y * w + x]
        total = row.sum()
        return (row / torch.where(total == 0, torch.ones_like(total), total)).reshape(h, w)

    def propagate(self, maps: torch.Tensor, iterations: int = 1) -> torch.Tensor:
        """``iterations`` rounds of ``m <- matrix() @ m`` on f32 ``maps`` [N, h, w] for any N (``engine.affinity_propagate``: blocks of
        32 maps, one launch per iteration and block)."""
        if maps.dim() != 3 or tuple(maps.shape[1:]) != self.grid:
            got = ' x '.join(str(int(s)) for s in maps.shape[-2:])
            raise ValueError(f'the affinity is of a grid of {self.grid[0]} x {self.grid[1]} cells, the maps are {got}')
        return _engine.affinity_propagate(self.sums, maps, iterations)

    def discover(self, anchors=16, threshold: float = 1.1, iterations: int = 3, size=None) -> 'Discovery':
        """Segments without a word list, in the DiffSeg manner (``libdaam_discover.so``): cells whose attention maps are
        close in symmetric KL divergence are merged into proposals, proposals are merged again, and every pixel takes the proposal
        that is largest there.

        1. ``engine.discover_prepare`` turns ``sums`` into probability rows ``P`` and their logarithms.
        2. ``anchors`` x ``anchors`` cells (a count per side, or a ``(rows, columns)`` pair; anchor ``(r, c)`` is the cell
           ``floor((r + 1/2) h / rows), floor((c + 1/2) w / columns)``) are compared with every cell (``engine.discover_pair_kl``); an
           anchor's proposal is the mean (``engine.discover_merge``) of the rows of the cells closer than ``threshold`` and of its own.
        3. ``iterations - 1`` times: the proposals are prepared and compared with each other, the matrix goes to the host (the one
           synchronisation of a round), ``discover_groups`` joins them greedily in list order, and the groups are merged.
        4. ``engine.discover_labels`` resizes the proposals to ``size`` -- an image (its ``size`` is read as ``(W, H)``), an ``(H, W)``
           pair, or ``None`` for the grid -- and labels every pixel.

        ``ValueError`` for ``threshold <= 0``, ``iterations < 1``, an anchor count below 1 and more than 255 proposals left."""
        threshold, iterations = float(threshold), int(iterations)
        if not threshold > 0:
            raise ValueError(f'threshold {threshold}: above 0')
        if iterations < 1:
            raise ValueError(f'iterations {iterations}: at least 1')
        h, w = self.grid
        cells = discover_anchors(self.grid, anchors)
        if size is None:
            out_h, out_w = h, w
        elif hasattr(size, 'size') and not isinstance(size, torch.Tensor):
            out_w, out_h = (int(v) for v in size.size)
        else:
            out_h, out_w = (int(v) for v in size)
        if not (1 <= out_h <= _engine.MAX_DISCOVER_OUT and 1 <= out_w <= _engine.MAX_DISCOVER_OUT):
            raise ValueError(f'size {out_h} x {out_w}: 1..{_engine.MAX_DISCOVER_OUT} a side')
        if len(cells) > _engine.MAX_DISCOVER_GROUPS:
            raise ValueError(f'{len(cells)} anchors: at most {_engine.MAX_DISCOVER_GROUPS}')
        sums = self.sums if self.sums.dtype == torch.float32 else self.sums.float()
        p, l = _engine.discover_prepare(sums)
        idx = torch.as_tensor(cells, dtype=torch.int64, device=p.device)
        d = _engine.discover_pair_kl(p[idx].contiguous(), l[idx].contiguous(), p, l)
        member = (d < threshold).to(torch.uint8)
        member[torch.arange(len(cells), device=p.device), idx] = 1            # an anchor always holds its own cell
        props, _ = _engine.discover_merge(p, member)
        for _ in range(iterations - 1):
            pp, lp = _engine.discover_prepare(props)
            groups = discover_groups(_engine.discover_pair_kl(pp, lp, pp, lp).cpu(), threshold)
            if len(groups) > _engine.MAX_DISCOVER_GROUPS:
                raise ValueError(f'{len(groups)} proposals are left: merging takes at most {_engine.MAX_DISCOVER_GROUPS}')
            member = torch.zeros(len(groups), props.shape[0], dtype=torch.uint8)
            for k, group in enumerate(groups):
                member[k, group] = 1
            props, _ = _engine.discover_merge(pp, member.to(p.device))
        if props.shape[0] > _engine.MAX_DISCOVER_PROPOSALS:
            raise ValueError(f'{props.shape[0]} proposals are left after {iterations} iterations: a label map orders at most '
                             f'{_engine.MAX_DISCOVER_PROPOSALS}; raise iterations or the threshold, or lower anchors')
        props = props.view(-1, h, w)
        return Discovery(props, _engine.discover_labels(props, out_h, out_w))

    def cpu(self) -> 'SelfAffinity':
        return SelfAffinity(self.sums.cpu(), self.grid, self.slices, self.calls)


def discover_anchors(grid: Tuple[int, int], anchors) -> List[int]:
    """The cells ``y w + x`` of the anchors of ``SelfAffinity.discover`` on a grid of ``h x w``, row-major: ``anchors`` is a count per
    side or a ``(rows, columns)`` pair, anchor ``(r, c)`` sits at ``floor((r + 1/2) h / rows)`` / ``floor((c + 1/2) w / columns)``,
    clipped to the grid."""
    h, w = int(grid[0]), int(grid[1])
    rows, cols = (anchors, anchors) if isinstance(anchors, int) else (int(v) for v in anchors)
    if rows < 1 or cols < 1:
        raise ValueError(f'anchors {anchors!r}: at least one per side')
    ys = [min(((2 * r + 1) * h) // (2 * rows), h - 1) for r in range(rows)]
    xs = [min(((2 * c + 1) * w) // (2 * cols), w - 1) for c in range(cols)]
    return [y * w + x for y in ys for x in xs]


def discover_groups(d, threshold: float) -> List[List[int]]:
    """The greedy pass of ``SelfAffinity.discover`` on the host: ``d`` [K, K] (a tensor or nested lists) is walked in list order; the
    first unused proposal takes every unused one with ``d[first][other] < threshold`` into its group, and they are marked used."""
    rows = d.tolist() if hasattr(d, 'tolist') else [list(r) for r in d]
    used = [False] * len(rows)
    groups = []
    for i, row in enumerate(rows):
        if used[i]:
            continue
        group = [i] + [j for j in range(len(rows)) if j != i and not used[j] and row[j] < threshold]
        for j in group:
            used[j] = True
        groups.append(group)
    return groups


class Discovery:
    """What ``SelfAffinity.discover`` found: ``proposals`` f32 [K, h, w], the merged attention maps, and ``labels`` uint8 [H, W], at
    every pixel the proposal that is largest there.  ``n`` = K; a proposal that wins no pixel has an area of 0."""

    def __init__(self, proposals: torch.Tensor, labels: torch.Tensor):
        self.proposals, self.labels = proposals, labels
        self.n = int(proposals.shape[0])
        self._masks: Optional[torch.Tensor] = None

    @property
    def areas(self) -> torch.Tensor:
        """int64 [K]: the pixels of every segment."""
        return torch.bincount(self.labels.reshape(-1).long(), minlength=self.n)

    @property
    def masks(self) -> torch.Tensor:
        """uint8 [K, H, W], built on the first use: ``masks[k] = labels == k``; they sum to 1 at every pixel."""
        if self._masks is None:
            ks = torch.arange(self.n, device=self.labels.device, dtype=self.labels.dtype)
            self._masks = (self.labels[None] == ks[:, None, None]).to(torch.uint8)
        return self._masks

    def mask(self, k: int) -> torch.Tensor:
        if not 0 <= int(k) < self.n:
            raise ValueError(f'segment {k}: 0..{self.n - 1}')
        return self.masks[int(k)]

    def _owners(self, ghm: 'GlobalHeatMap', words) -> List[Optional[int]]:
        """Per segment the index of the word of ``words`` that puts most attention inside it; ``None`` for a segment without a pixel
        or without any attention."""
        if not words:
            raise ValueError('names needs at least one word')
        values, indices = ghm.attribute(self.masks).top_words(words)
        values, indices, areas = values[:, 0].tolist(), indices[:, 0].tolist(), self.areas.tolist()
        return [i if a > 0 and v > 0 else None for v, i, a in zip(values, indices, areas)]

    def names(self, ghm: 'GlobalHeatMap', words: Sequence[Union[str, Tuple[str, Optional[int]]]]) -> List[Optional[str]]:
        """One word of ``words``, or ``None``, per segment: ``ghm.attribute(masks).top_words(words)``."""
        names = [w if isinstance(w, str) else w[0] for w in words]
        return [None if i is None else names[i] for i in self._owners(ghm, words)]

    def word_masks(self, ghm: 'GlobalHeatMap', words: Sequence[Union[str, Tuple[str, Optional[int]]]]) -> torch.Tensor:
        """uint8 [len(words), H, W]: the union of the segments each word owns -- the shape ``evaluate.mask_overlap_matrix``,
        ``evaluate.mask_components`` and ``Segmentation.iou`` take."""
        owners = self._owners(ghm, words)
        table = torch.zeros(len(words), self.n, dtype=torch.uint8)
        for k, i in enumerate(owners):
            if i is not None:
                table[i, k] = 1
        return table.to(self.labels.device)[:, self.labels.long()]

    def cpu(self) -> 'Discovery':
        return Discovery(self.proposals.cpu(), self.labels.cpu())


class GlobalHeatMap:
    """reference heatmap.py:114-142."""

    def __init__(self, tokenizer: Any, prompt: str, heat_maps: torch.Tensor):
        self.tokenizer = tokenizer
        self.heat_maps = heat_maps
        self.prompt = prompt
        self.compute_word_heat_map = lru_cache(maxsize=50)(self.compute_word_heat_map)

    def compute_word_heat_map(self, word: str, word_idx: Optional[int] = None, offset_idx: int = 0) -> WordHeatMap:
        merge_idxs, word_idx = compute_token_merge_indices(self.tokenizer, self.prompt, word, word_idx, offset_idx)
        return WordHeatMap(_engine.word_heat_map(self.heat_maps, merge_idxs), word, word_idx)

    def segment(self, words: Sequence[Union[str, Tuple[str, Optional[int]]]], image, threshold: float = 0.4, absolute: bool = False,
                labels: bool = True) -> Segmentation:
        """``compute_word_heat_map(w).expand_as(image, threshold=) > threshold`` for every ``w`` of ``words`` (strings, or
        ``(word, word_idx)`` pairs) and the label map over them, in three launches per 32 words (``engine.word_masks``) with the
        results left on the device.  The output size follows ``WordHeatMap.expand_as``.  A label map orders at most 32 words:
        more are a ``ValueError`` unless ``labels=False``, which serves the masks in chunks."""
        pairs = [(w, None) if isinstance(w, str) else (w[0], w[1]) for w in words]
        if not pairs:
            raise ValueError('segment needs at least one word')
        if labels and len(pairs) > _engine.MAX_MASK_WORDS:
            raise ValueError(f'a label map orders at most {_engine.MAX_MASK_WORDS} words, got {len(pairs)}; pass labels=False for masks only')
        resolved = [compute_token_merge_indices(self.tokenizer, self.prompt, w, i) for w, i in pairs]
        maps = self.heat_maps
        size = (image.size[0], image.size[1]) if maps.shape[-2] == maps.shape[-1] else (image.size[1], image.size[0])
        chunks, count = [[]], 0
        for idxs, _ in resolved:                 # a call takes 32 words and 255 indices
            if len(chunks[-1]) == _engine.MAX_MASK_WORDS or count + len(idxs) > _engine.MAX_MASK_INDICES:
                chunks.append([])
                count = 0
            chunks[-1].append(idxs)
            count += len(idxs)
        if labels and len(chunks) > 1:
            raise ValueError(f'a label map takes at most {_engine.MAX_MASK_INDICES} token indices over all words; pass labels=False')
        word_maps, masks, label_map = [], [], None
        for chunk in chunks:
            wm, mk, label_map = _engine.word_masks(maps, chunk, int(size[0]), int(size[1]), absolute=absolute, threshold=threshold,
                                                   labels=labels)
            word_maps.append(wm)
            masks.append(mk)
        planes = [plane for wm in word_maps for plane in wm]
        heat = [WordHeatMap(plane, w, r[1]) for plane, (w, _), r in zip(planes, pairs, resolved)]
        return Segmentation([w for w, _ in pairs], heat, masks[0] if len(masks) == 1 else torch.cat(masks), label_map)

    def refine(self, words: Sequence[Union[str, Tuple[str, Optional[int]]]], image, threshold: float = 0.4, iterations: int = 10,
               dilations=_engine.REFINE_DILATIONS, scale: float = 0.1, absolute: bool = False, labels: bool = True,
               affinity=None) -> Segmentation:
        """``segment`` with the image's outline: the soft map ``compute_word_heat_map(w).expand_as(image, absolute=)`` of every word is
        propagated for ``iterations`` rounds along the local colour affinities of ``image`` (a PIL image: each pixel takes the
        affinity-weighted mean of its 8 neighbours at every dilation; ``engine.refine_affinity`` / ``refine_maps``) and
        then thresholded.  The result is a ``Segmentation`` whose ``refined`` holds the f32 maps, so ``iou`` / ``ioa`` / ``components`` /
        ``clean`` / ``attribute`` compose as after ``segment``.  ``affinity``: an ``ImageAffinity`` of this image
        (``daam_amd.image_affinity``) to reuse across calls; ``dilations`` and ``scale`` are then its own.  The maps are not
        renormalised after the propagation."""
        pairs = [(w, None) if isinstance(w, str) else (w[0], w[1]) for w in words]
        if not pairs:
            raise ValueError('refine needs at least one word')
        resolved = [compute_token_merge_indices(self.tokenizer, self.prompt, w, i) for w, i in pairs]
        planes = _engine.word_maps(self.heat_maps, [idxs for idxs, _ in resolved])
        heat = [WordHeatMap(plane, w, r[1]) for plane, (w, _), r in zip(planes, pairs, resolved)]
        return _refine_words([w for w, _ in pairs], heat, image, threshold, iterations, dilations, scale, absolute, labels, affinity)

    def propagate(self, affinity: SelfAffinity, iterations: int = 1) -> 'GlobalHeatMap':
        """A new ``GlobalHeatMap`` (same tokenizer and prompt) whose every token plane is propagated along the generation's
        self-attention affinity for ``iterations`` rounds (``SelfAffinity.propagate``), computed in f32 and cast back to the planes'
        dtype.  The propagation is linear, so ``compute_word_heat_map`` on the result is the propagated word map, and ``segment``,
        ``threshold_sweep``, ``localize``, ``refine`` and ``attribute`` compose on it unchanged."""
        if not isinstance(affinity, SelfAffinity):
            raise TypeError(f'affinity must be a SelfAffinity, got {type(affinity).__name__}')
        maps = self.heat_maps
        if maps.dim() != 3 or tuple(maps.shape[1:]) != affinity.grid:
            mine = ' x '.join(str(int(s)) for s in maps.shape[-2:])
            raise ValueError(f'the affinity is of a grid of {affinity.grid[0]} x {affinity.grid[1]} cells, the heat maps are {mine}')
        out = affinity.propagate(maps.float().contiguous(), iterations)
        return GlobalHeatMap(self.tokenizer, self.prompt, out.to(maps.dtype))

    def threshold_sweep(self, words: Sequence[Union[str, Tuple[str, Optional[int]]]], image,
                        truth: Union[None, torch.Tensor, Segmentation] = None, thresholds=None, absolute: bool = False) -> ThresholdSweep:
        """``segment(words, image, threshold=t).overlaps(truth)`` for every ``t`` of ``thresholds`` (default 0, 0.05 .. 1) at the cost
        of about one ``segment`` call (``engine.threshold_sweep``: the expansion is the same at every threshold, only a comparison
        changes).  Words are resolved as in ``segment`` and the output is sized as in ``expand_as``; ``truth`` is a mask [H, W], a
        stack [G, H, W] of that size (uint8 / bool as they are, other dtypes through ``!= 0``) or a ``Segmentation``; ``None``
        leaves the predicted areas alone (G = 0)."""
        pairs = [(w, None) if isinstance(w, str) else (w[0], w[1]) for w in words]
        if not pairs:
            raise ValueError('threshold_sweep needs at least one word')
        resolved = [compute_token_merge_indices(self.tokenizer, self.prompt, w, i) for w, i in pairs]
        maps = self.heat_maps
        size = (image.size[0], image.size[1]) if maps.shape[-2] == maps.shape[-1] else (image.size[1], image.size[0])
        thresholds = [i / 20 for i in range(21)] if thresholds is None else thresholds
        masks = truth.masks if isinstance(truth, Segmentation) else truth
        planes = _engine.word_maps(maps, [idxs for idxs, _ in resolved])
        pred, inter, area = _engine.threshold_sweep(planes, int(size[0]), int(size[1]), thresholds, masks, absolute=absolute)
        thr = torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1).to(pred.device)
        if inter is None:
            inter = torch.zeros(pred.shape[0], 0, pred.shape[1], dtype=torch.int32, device=pred.device)
            area = torch.zeros(0, dtype=torch.int32, device=pred.device)
        return ThresholdSweep([w for w, _ in pairs], thr, inter, pred, area)

    def localize(self, words: Sequence[Union[str, Tuple[str, Optional[int]]]], image, thresholds=(0.4,),
                 truth: Union[None, torch.Tensor, Segmentation] = None, absolute: bool = False, component: Optional[str] = None,
                 connectivity: int = 8) -> Localization:
        """The bounding box of ``segment(words, image, threshold=t).masks`` for every ``t`` of ``thresholds``, the peak of every
        word's expanded map and, with ``truth`` (a mask [H, W], a stack [G, H, W] or a ``Segmentation``), the truth masks' boxes and
        the pointing hits -- one pass at image resolution (``engine.localize``), no mask is written.  Words are resolved as in
        ``segment`` and the output is sized as in ``expand_as``.

        ``component='largest'``: ``boxes[j][t]`` is the box of the LARGEST connected component (``connectivity`` 4 or 8) of that
        mask, as CAM-style CorLoc is defined, so a stray speckle no longer stretches the box.  The row and column maxima of the
        one-pass route cannot give that box (they say which rows and columns hold a mask pixel, not which pixels touch), so per
        threshold the masks are written (``engine.word_masks``) and labelled (``engine.mask_components``); peaks, peak values,
        truth boxes and hits still come from one ``engine.localize`` call."""
        pairs = [(w, None) if isinstance(w, str) else (w[0], w[1]) for w in words]
        if not pairs:
            raise ValueError('localize needs at least one word')
        if component not in (None, 'largest'):
            raise ValueError(f"component {component!r}: None or 'largest'")
        resolved = [compute_token_merge_indices(self.tokenizer, self.prompt, w, i) for w, i in pairs]
        maps = self.heat_maps
        size = (image.size[0], image.size[1]) if maps.shape[-2] == maps.shape[-1] else (image.size[1], image.size[0])
        masks = truth.masks if isinstance(truth, Segmentation) else truth
        planes = _engine.word_maps(maps, [idxs for idxs, _ in resolved])
        if component == 'largest':
            thr = torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1)
            _, peaks, values, truth_boxes, hits = _engine.localize(planes, int(size[0]), int(size[1]), (), masks, absolute=absolute)
            cols = [_engine.mask_components(self.segment(pairs, image, threshold=float(t), absolute=absolute, labels=False).masks,
                                            connectivity, max_components=0, labels=False)[3][:, 2:6] for t in thr]
            boxes = torch.stack(cols, 1) if cols else torch.zeros(len(pairs), 0, 4, dtype=torch.int32, device=peaks.device)
            return Localization([w for w, _ in pairs], thr.to(peaks.device), (int(size[0]), int(size[1])), boxes, peaks, values, truth_boxes, hits)
        boxes, peaks, values, truth_boxes, hits = _engine.localize(planes, int(size[0]), int(size[1]), thresholds, masks, absolute=absolute)
        thr = torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1).to(boxes.device)
        return Localization([w for w, _ in pairs], thr, (int(size[0]), int(size[1])), boxes, peaks, values, truth_boxes, hits)

    def attribute(self, regions: Union[torch.Tensor, Segmentation]) -> RegionAttribution:
        """The opposite question to ``segment``: for each region -- ``regions`` is a mask [H, W], a stack [M, H, W] (uint8 / bool as
        they are, other dtypes through ``!= 0``) or a ``Segmentation`` (its ``.masks``) -- how much of every token row's expanded
        heat map lies inside it (``engine.region_scores``: one pass over the mask bytes, no plane at image resolution).  The
        target size is the masks' own ``[H, W]``, taken as it is, which is how ``Segmentation.masks`` is laid out: no PIL-order
        swap happens here (``expand_as`` / ``segment`` apply theirs when they read ``image.size``)."""
        masks = regions.masks if isinstance(regions, Segmentation) else regions
        scores, area, footprint = _engine.region_scores(self.heat_maps, masks)
        return RegionAttribution(scores, area, footprint, self.tokenizer, self.prompt)

    def coattention(self) -> torch.Tensor:
        """f32 [rows, rows]: the Gram matrix of the map's token rows, ``out[i][j] = sum_p heat_maps[i][p] * heat_maps[j][p]``
        (``engine.map_gram``: the library call of ``compute_key_coattention`` on the global map as one key)."""
        return _engine.map_gram(self.heat_maps)

    def word_cosine(self, word_a: str, word_b: str, eps: float = 1e-12) -> float:
        """The cosine of two words' maps (``compute_word_heat_map``: the mean of the word's token rows) from block means of
        ``coattention()``: a threshold-free companion of ``WordHeatMap.compute_ioa``.  A word whose map is all zeros gives 0."""
        a, _ = compute_token_merge_indices(self.tokenizer, self.prompt, word_a, None)
        b, _ = compute_token_merge_indices(self.tokenizer, self.prompt, word_b, None)
        g = self.coattention().double()

        def block(r, c):
            return float(g[list(r)][:, list(c)].mean())
        return block(a, b) / (block(a, a) * block(b, b) + eps) ** 0.5

    def parsed_heat_maps(self) -> Iterable[ParsedHeatMap]:
        """One ``ParsedHeatMap`` per token of the parsed prompt whose text is found among the prompt's tokenizer tokens
        (heatmap.py:125-131; the others are skipped)."""
        for token in cached_nlp(self.prompt):
            try:
                yield ParsedHeatMap(self.compute_word_heat_map(token.text), token)
            except ValueError:
                continue

    def dependency_relations(self) -> Iterable[SyntacticHeatMapPair]:
        """One pair per non-root token: the maps of the token and of its syntactic head (heatmap.py:133-142)."""
        for token in cached_nlp(self.prompt):
            if token.dep_ == 'ROOT':
                continue
            try:
                dependent = self.compute_word_heat_map(token.text)
                head = self.compute_word_heat_map(token.head.text)
            except ValueError:
                continue
            yield SyntacticHeatMapPair(head, dependent, token.head.text, token.text, token.dep_)
