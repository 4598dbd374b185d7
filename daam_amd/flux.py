"""``trace_flux``: heat maps for FLUX-class pipelines, whose transformer rotates Q and K (RoPE) and has, after its double-stream
(MMDiT) blocks, single-stream blocks in which one sequence ``[text; image]`` attends to itself.  The DAAM quantity is that of
``trace_joint`` -- the image-to-text block of the joint softmax, with the image keys in the denominator
(``daam_joint_tap_accumulate``) -- read off the ROTATED Q and K, which ``daam_rope_apply`` (include/daam_rope.h,
DESIGN 3.25) produces bit for bit as the model's own attention sees them.

The protocol the hooker relies on is that of diffusers' ``FluxAttnProcessor2_0``:

    attn.heads, attn.scale, attn.processor, attn.set_processor(p)
    processor(attn, hidden_states, encoder_hidden_states=None, attention_mask=None, image_rotary_emb=None)
    image_rotary_emb = (cos, sin)        f32 [T + P, d], text rows first; rotation in diffusers' interleaved-pair form
                                         apply_rotary_emb(x, (cos, sin), use_real=True, use_real_unbind_dim=-1), after the norms

  double-stream   ``pipe.transformer.transformer_blocks[*].attn``, called with ``encoder_hidden_states=ctx`` [1, T, C] and
                  ``hidden_states`` [1, P, C]:
                      q     = attn.norm_q(attn.to_q(hidden_states))               rotated by table rows [T, T + P)
                      k_img = attn.norm_k(attn.to_k(hidden_states))               rotated by table rows [T, T + P)
                      k_txt = attn.norm_added_k(attn.add_k_proj(ctx))             rotated by table rows [0, T)
                  tapped when ctx is given, the mask is None, P is the grid's cell count and the table has T + P rows.  One
                  ``rope_apply`` of three jobs into one reused [1, T + 2 P, C] buffer; the text queries are never projected.
  single-stream   ``pipe.transformer.single_transformer_blocks[*].attn``, called with ``encoder_hidden_states=None`` and
                  ``hidden_states`` = x [1, T + P, C], text rows first:
                      q = attn.norm_q(attn.to_q(x[:, T:]))                        the image rows alone, table rows [T, T + P)
                      k = attn.norm_k(attn.to_k(x))                               all rows, the whole table
                  tapped when T = rows - cells is in 1..512, the table has T + P rows and the mask is None -- and, where the
                  double-stream blocks are hooked too, T is the text length their calls of this generation were tapped with (a
                  sequence of another grid is then left alone, not read with a wrong T).  Two jobs; the tap reads k[:, :T] and
                  k[:, T:] as views of the rotated buffer, with no copy.

each norm acting on the head dim of ``[batch, rows, heads, d]`` and skipped where the attribute is ``None``.  With
``image_rotary_emb=None`` there is no rotary pass and the tap reads the projections.  FLUX runs no ``[uncond; cond]`` batch: a batch of
1 is tapped whole, a tapped call with a larger batch is a ``ValueError``.  The prompt comes from ``pipe.check_inputs(prompt, prompt_2,
...)``: T5 (``pipe.tokenizer_2``) encodes ``prompt_2`` where it is given, else ``prompt``; the context holds T5 rows alone.
``trace()`` / ``trace_joint()`` are untouched by this module; nothing is located or allocated unless ``trace_flux`` is used.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import engine as _engine
from .heatmap import GlobalHeatMap, SelfAffinity
from .hook import AggregateHooker, ObjectHooker
from .joint import JointAttentionHooker, _head_dim, _self_affinity_of, _transformer_dtype

__all__ = ['trace_flux', 'FluxHeatMapHooker', 'T5RowTokenizer']

WORD_MARK = '▁'                                 # sentencepiece's word-start marker
KINDS = ('double', 'single')


class T5RowTokenizer:
    """What ``compute_token_merge_indices`` needs of a tokenizer, over a sentencepiece (T5) one.  Sentencepiece marks where a word
    STARTS (``▁dog``, ``s``); the lookup compares bare pieces and tells 'dog' from the first piece of 'dogs' by where a word ENDS, as
    CLIP's vocabulary does.  So ``tokenize`` strips the word marker from every piece and puts it BEHIND a piece that the next piece
    continues: 'a dogs bench' gives ``a``, ``dog▁``, ``s``, ``bench``.  One piece stays one entry -- a marker that is a piece of its own
    (T5 emits one before some punctuation) becomes an empty entry that no word's pieces match, it is not taken out --, so T5 token
    ``i`` lives in row ``i + 1`` of a heat map whose row 0 stands where CLIP's start-of-text row stands."""

    def __init__(self, tokenizer):
        self.tokenizer = tokenizer

    def tokenize(self, text: str) -> List[str]:
        pieces = list(self.tokenizer.tokenize(text))
        starts = [piece.startswith(WORD_MARK) for piece in pieces] + [True]
        return [piece.replace(WORD_MARK, '') + ('' if starts[i + 1] else WORD_MARK) for i, piece in enumerate(pieces)]

    def __getattr__(self, name):
        return getattr(self.tokenizer, name)


class FluxHeatMapHooker(AggregateHooker):
    """``with trace_flux(pipe) as tc: pipe(prompt); tc.compute_global_heat_map()``.

    Every tapped attention call (module docstring) adds the text columns of its joint softmax, on the rotated Q and K, to one f32
    ``[T, h w]`` tensor, T the number of T5 rows (``per_head=True``: to one plane per head).  The generation itself is bit-identical
    to the untraced one.

    ``height`` / ``width``: the size of the generation in pixels; ``cell``: the pixels a token covers on a side (the VAE's factor 8
    times the 2 x 2 packing of FLUX's latents); ``blocks``: ``'all'``, ``'double'`` or ``'single'``, the kind of block that is hooked.

    ``self_affinity=True``: every tapped call, double-stream or single-stream, also adds the IMAGE columns of the same
    softmax to one f32 ``[h w, h w]`` matrix, on the same stream, from the same ROTATED Q and image K and the statistics the tap has
    just written; ``compute_self_affinity()`` returns it as a ``SelfAffinity``.  One thing differs from the UNet: a row sums to
    ``slices`` MINUS the mass the cell gave to the text keys (``matrix()``, ``of()`` and ``propagate()`` divide by the row sum, so they
    hold as they are).  Without the option nothing of it is loaded or allocated."""

    def __init__(self, pipeline, per_head: bool = False, height: int = 1024, width: int = 1024, cell: int = 16, blocks: str = 'all',
                 self_affinity: bool = False):
        transformer = getattr(pipeline, 'transformer', None)
        if transformer is None or not hasattr(transformer, 'single_transformer_blocks') or not hasattr(transformer, 'transformer_blocks'):
            raise ValueError('trace_flux needs a pipeline with a `transformer` of `transformer_blocks` and `single_transformer_blocks` '
                             '(FLUX class); SD3-class pipelines are traced with `trace_joint`, UNet pipelines with `trace`')
        if blocks not in ('all',) + KINDS:
            raise ValueError(f"trace_flux: blocks {blocks!r}: 'all', 'double' or 'single'")
        dtype = _transformer_dtype(transformer)
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f'trace_flux reads fp16 or bf16 Q and K: the pipeline\'s transformer is {dtype}')
        self.pipe = pipeline
        self.per_head = bool(per_head)
        height, width, cell = int(height), int(width), int(cell)
        if cell < 1 or height % cell or width % cell:
            raise ValueError(f'a generation of {height} x {width} pixels is no whole number of {cell}-pixel cells')
        self.grid = (height // cell, width // cell)
        self.cells = self.grid[0] * self.grid[1]
        if not 1 <= self.cells <= _engine.MAX_JOINT_CELLS:
            raise ValueError(f'a grid of {self.grid[0]} x {self.grid[1]} cells: the joint tap takes 1..{_engine.MAX_JOINT_CELLS} cells')
        located = {'double': [block.attn for block in transformer.transformer_blocks] if blocks in ('all', 'double') else [],
                   'single': [block.attn for block in transformer.single_transformer_blocks] if blocks in ('all', 'single') else []}
        for attn in located['double'] + located['single']:
            if _head_dim(attn) not in _engine.JOINT_HEAD_DIMS:
                raise ValueError(f'trace_flux: head dim {_head_dim(attn)}: one of {_engine.JOINT_HEAD_DIMS}')
        self.state: Optional[_engine.JointTapState] = None      # made by the first tapped call, which knows the context length
        self.affinity = _engine.JointAffinityState(*self.grid) if self_affinity else None
        self.table = _engine.RopeTable()
        self.last_prompt: str = ''
        self._calls: Dict[str, int] = dict.fromkeys(KINDS, 0)
        self.hooks_double = bool(located['double'])
        self._tokens: Optional[int] = None                      # the text rows of this generation's tapped double-stream calls
        self._rotated: Optional[torch.Tensor] = None            # [1, T + 2 P, C], reused by every tapped call
        super().__init__([_FluxPipelineHooker(pipeline, self)] + [FluxAttentionHooker(attn, self, kind) for kind in KINDS for attn in located[kind]])

    # -- fed by the hookers ----------------------------------------------------------------------------------------------------------
    def _begin_generation(self, prompt) -> None:
        self.last_prompt = prompt if isinstance(prompt, str) else prompt[0]
        self.table.reset()
        self._calls = dict.fromkeys(KINDS, 0)
        self._tokens = None
        if self.state is not None:
            self.state.reset()
        if self.affinity is not None:
            self.affinity.reset()

    def _buffer(self, like: torch.Tensor, rows: int) -> torch.Tensor:
        buf = self._rotated
        if buf is None or buf.shape[1] < rows or buf.shape[2] != like.shape[2] or buf.dtype != like.dtype or buf.device != like.device:
            buf = self._rotated = torch.empty(1, rows, like.shape[2], dtype=like.dtype, device=like.device)
        return buf

    def _tap(self, kind: str, q, k_txt, k_img, heads: int, scale: float) -> None:
        if self.state is None or self.state.tokens != k_txt.shape[1]:
            self.state = _engine.JointTapState(self.grid[0], self.grid[1], k_txt.shape[1], self.per_head)
        self.state.tap(q, k_txt, k_img, heads, scale)
        if self.affinity is not None:
            self.affinity.tap(q, k_img, heads, scale, self.state.stats)
        self._calls[kind] += 1
        if kind == 'double':
            self._tokens = k_txt.shape[1]

    # -- results ---------------------------------------------------------------------------------------------------------------------
    def _sums(self) -> torch.Tensor:
        if self.state is None or self.state.sums is None or not self.state.calls:
            raise RuntimeError('No heat maps found. Did you forget to call `with trace_flux(...)` during generation?')
        return self.state.sums

    def calls_by_kind(self) -> Dict[str, int]:
        """``{'double': n, 'single': m}``: the tapped calls of the last generation."""
        return dict(self._calls)

    def raw_heat_maps(self) -> torch.Tensor:
        """The running sums of the T context rows as f32 ``[T, h, w]``: the sum over tapped calls and heads."""
        sums = self._sums()
        plane = sums.sum(dim=0) if self.per_head else sums.clone()
        return plane.view(-1, *self.grid)

    def compute_global_heat_map(self, prompt: Optional[str] = None) -> GlobalHeatMap:
        """The mean over tapped calls and heads as a ``GlobalHeatMap`` over T5 rows: f32 ``[1 + T, h, w]`` whose row 0 is a zero plane
        where CLIP's start-of-text row stands, with a ``T5RowTokenizer`` over ``pipe.tokenizer_2`` -- ``compute_word_heat_map`` /
        ``segment`` / ``localize`` / ... apply as on a UNet trace."""
        maps = self.raw_heat_maps() / float(self.state.slices)
        maps = torch.cat([torch.zeros_like(maps[:1]), maps], dim=0)
        return GlobalHeatMap(T5RowTokenizer(self.pipe.tokenizer_2), self.last_prompt if prompt is None else prompt, maps.contiguous())

    def compute_head_heat_maps(self) -> torch.Tensor:
        """f32 ``[heads, T, h, w]`` (a trace built with ``per_head=True``): per head the mean over tapped calls."""
        if not self.per_head:
            raise ValueError('the trace was built without per_head=True')
        sums = self._sums()
        return (sums / float(self.state.slices // self.state.heads)).view(sums.shape[0], sums.shape[1], *self.grid)

    def compute_self_affinity(self) -> SelfAffinity:
        """The image-to-image affinity of the last generation (a trace built with ``self_affinity=True``): the image columns of the
        joint softmax on the rotated Q and K, summed over every tapped call and head (a copy: the next generation starts over)."""
        return _self_affinity_of(self.affinity, 'trace_flux')


class _FluxPipelineHooker(ObjectHooker):
    """A ``pipe(prompt)`` call starts a new generation: the prompt T5 encodes is remembered, the next tapped call overwrites the sums."""

    def __init__(self, pipeline, parent: FluxHeatMapHooker):
        super().__init__(pipeline)
        self.parent = parent

    def _hook_impl(self):
        self.monkey_patch('check_inputs', self._before_generation)

    def _before_generation(self, _pipe, *args, **kwargs):
        prompt = args[0] if args else kwargs.get('prompt')
        prompt_2 = args[1] if len(args) > 1 else kwargs.get('prompt_2')
        for p in (prompt, prompt_2):
            if p is not None and not isinstance(p, str) and len(p) > 1:
                raise ValueError('Only single prompt generation is supported for heat map computation.')
        read = prompt_2 if prompt_2 else prompt
        self.parent._begin_generation(read if read else '')
        return self.monkey_super('check_inputs', *args, **kwargs)


class FluxAttentionHooker(ObjectHooker):
    """The processor installed on every located ``attn``.  The model's output is what the ORIGINAL processor returns for the original
    arguments, so the traced generation is bit-identical to the untraced one.  Beside it, under ``no_grad``, a call that fits the
    protocol of its kind (module docstring) is projected, rotated and tapped."""

    _project = staticmethod(JointAttentionHooker._project)

    def __init__(self, module, parent: FluxHeatMapHooker, kind: str):
        super().__init__(module)
        self.parent = parent
        self.kind = kind

    def _hook_impl(self):
        self.original_processor = self.module.processor
        self.module.set_processor(self)

    def _unhook_impl(self):
        self.module.set_processor(self.original_processor)

    def __call__(self, attn, hidden_states, *args, **kwargs):
        out = self.original_processor(attn, hidden_states, *args, **kwargs)
        context = kwargs.get('encoder_hidden_states', args[0] if args else None)
        mask = kwargs.get('attention_mask', args[1] if len(args) > 1 else None)
        rotary = kwargs.get('image_rotary_emb', args[2] if len(args) > 2 else None)
        if mask is not None or not torch.is_tensor(hidden_states) or hidden_states.dim() != 3:
            return out
        cells = self.parent.cells
        if self.kind == 'double':
            if context is None or hidden_states.shape[1] != cells or not 1 <= context.shape[1] <= _engine.MAX_JOINT_TOKENS:
                return out
            tokens = context.shape[1]
        else:
            tokens = hidden_states.shape[1] - cells
            if context is not None or not 1 <= tokens <= _engine.MAX_JOINT_TOKENS:
                return out
            if self.parent.hooks_double and self.parent._tokens != tokens:
                return out                          # not the text length this generation's double-stream calls were tapped with
        if rotary is not None and (rotary[0].dim() != 2 or rotary[0].shape[0] != tokens + cells or rotary[1].shape != rotary[0].shape):
            return out
        if hidden_states.shape[0] != 1:
            raise ValueError(f'trace_flux: a batch of {hidden_states.shape[0]}: one prompt, one image per prompt')
        with torch.no_grad():
            self._tap(attn, hidden_states, context, rotary, tokens)
        return out

    def _tap(self, attn, x, context, rotary, T: int) -> None:
        parent, heads, P = self.parent, attn.heads, self.parent.cells
        norm_q, norm_k = getattr(attn, 'norm_q', None), getattr(attn, 'norm_k', None)
        if self.kind == 'double':
            q = self._project(attn.to_q, norm_q, x, heads)
            k_img = self._project(attn.to_k, norm_k, x, heads)
            k_txt = self._project(attn.add_k_proj, getattr(attn, 'norm_added_k', None), context, heads)
        else:
            q = self._project(attn.to_q, norm_q, x[:, T:], heads)
            k = self._project(attn.to_k, norm_k, x, heads)
            k_txt, k_img = k[:, :T], k[:, T:]
        if rotary is not None:
            d = q.shape[2] // heads
            cos, sin = parent.table.get(rotary[0]), parent.table.get(rotary[1])
            buf = parent._buffer(q, T + 2 * P)
            image = (cos[T:], sin[T:], heads)
            if self.kind == 'double':
                _engine.rope_apply([(q, buf[:, T + P:T + 2 * P], *image), (k_img, buf[:, T:T + P], *image),
                                    (k_txt, buf[:, :T], cos[:T], sin[:T], heads)], d)
            else:
                _engine.rope_apply([(q, buf[:, T + P:T + 2 * P], *image), (k, buf[:, :T + P], cos, sin, heads)], d)
            q, k_txt, k_img = buf[:, T + P:T + 2 * P], buf[:, :T], buf[:, T:T + P]
        parent._tap(self.kind, q, k_txt, k_img, heads, attn.scale)


trace_flux = FluxHeatMapHooker
