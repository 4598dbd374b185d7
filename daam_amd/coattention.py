"""Token co-attention (``DiffusionHeatMapHooker.compute_key_coattention``): which heads and layers entangle two words and which keep
them apart -- the reference's cohyponym / adjectival entanglement question (``heatmap.py:95-96`` on thresholded masks of the global
map), asked per ``(factor, layer, head)`` key and without a threshold.  The container holds one Gram matrix of token planes per key
(``daam_token_gram`` of ``libdaam_analysis.so``); everything below is small arithmetic on it."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from .heatmap import KeyAnalysis
from .utils import compute_token_merge_indices

__all__ = ['KeyCoattention']


@dataclass(init=False)
class KeyCoattention(KeyAnalysis):
    """``gram[k][i][j] = sum_p plane_k,i[p] * plane_k,j[p]`` of every selected key's raw running sums, at the key's own resolution (no
    bicubic, no clamp).  A word map is the mean of its token rows, so the Gram of two words is the mean of a block of ``gram``,
    exactly: one matrix per key answers every word pair.  On the device until ``cpu()``."""
    gram: torch.Tensor                          # f32 [K, rows, rows], bitwise symmetric
    eps: float = 1e-12                          # what ``of`` adds under its square root

    def __init__(self, keys, gram, layer_names=None, tokenizer=None, prompt=None, eps=1e-12):
        super().__init__(keys, layer_names, tokenizer, prompt)
        self.gram, self.eps = gram, eps

    def cosine(self, eps: float = 1e-12) -> torch.Tensor:
        """f32 [K, rows, rows]: ``gram[k][i][j] / sqrt(gram[k][i][i] * gram[k][j][j] + eps)``; a row of zeros gives 0, not NaN."""
        diag = torch.diagonal(self.gram, dim1=1, dim2=2)
        return self.gram / torch.sqrt(diag[:, :, None] * diag[:, None, :] + eps)

    def _rows_of(self, word: str, word_idx: Optional[int]) -> List[int]:
        idxs, _ = compute_token_merge_indices(self.tokenizer, self.prompt, word, word_idx)
        return list(idxs)

    def word_gram(self, word_a: str, word_b: str, word_idx_a: Optional[int] = None, word_idx_b: Optional[int] = None):
        """``(g_ab, g_aa, g_bb)``, each f64 [K]: the dot products of the two WORD maps (``compute_word_heat_map``'s merge: the mean of
        the word's token rows) per key, as block means of ``gram``."""
        a, b = self._rows_of(word_a, word_idx_a), self._rows_of(word_b, word_idx_b)
        g = self.gram.double()

        def block(r, c):
            return g[:, r][:, :, c].mean(dim=(1, 2))
        return block(a, b), block(a, a), block(b, b)

    def of(self, word_a: str, word_b: str, word_idx_a: Optional[int] = None, word_idx_b: Optional[int] = None) -> torch.Tensor:
        """f32 [K]: the cosine of the two word maps per key."""
        ab, aa, bb = self.word_gram(word_a, word_b, word_idx_a, word_idx_b)
        return (ab / torch.sqrt(aa * bb + self.eps)).to(torch.float32)

    def top_keys(self, word_a: str, word_b: str, k: int = 10, largest: bool = True):
        """The ``k`` keys that entangle the two words most (``largest=False``: least): ``[((factor, layer, head), cosine)]`` with the
        layer's name in place of its index when the trace's layer names are known; equal values keep the key order."""
        col = self.of(word_a, word_b).cpu()
        order = torch.sort(col, descending=largest, stable=True).indices[:k].tolist()
        names = self.layer_names

        def named(key):
            return key if names is None else (key[0], names[key[1]], key[2])
        return [(named(self.keys[i]), float(col[i])) for i in order]

    def _values(self, word_a, word_b, word_idx_a, word_idx_b) -> torch.Tensor:
        if (word_a is None) != (word_b is None):
            raise ValueError('pass both words, or neither (the token cosines)')
        return self.cosine() if word_a is None else self.of(word_a, word_b, word_idx_a, word_idx_b)

    def by_layer(self, word_a: Optional[str] = None, word_b: Optional[str] = None, word_idx_a: Optional[int] = None,
                 word_idx_b: Optional[int] = None):
        """``(layers, means)``: the mean over each layer's heads, layers ascending, as ``KeyScores.by_layer`` gives its own -- of the
        token cosines, f32 [len(layers), rows, rows], or with two words of their cosine, f32 [len(layers)]."""
        return self._grouped(1, self._values(word_a, word_b, word_idx_a, word_idx_b))

    def by_head(self, word_a: Optional[str] = None, word_b: Optional[str] = None, word_idx_a: Optional[int] = None,
                word_idx_b: Optional[int] = None):
        """``(heads, means)``: the mean over the layers that have the head, heads ascending; values as in ``by_layer``."""
        return self._grouped(2, self._values(word_a, word_b, word_idx_a, word_idx_b))

    def mean(self) -> torch.Tensor:
        """f32 [rows, rows]: the mean cosine over the keys."""
        return self.cosine().mean(dim=0)

    def cpu(self) -> 'KeyCoattention':
        return KeyCoattention(list(self.keys), self.gram.cpu(), self.layer_names, self.tokenizer, self.prompt, self.eps)
