"""``trace_joint``: heat maps for MMDiT pipelines (Stable Diffusion 3 / 3.5 class), whose transformer blocks have no cross-attention:
the image tokens attend to text AND image keys in one joint softmax.  The DAAM quantity is the image-to-text block of that matrix,
with the image keys in the denominator (``daam_joint_tap_accumulate``, include/daam_joint_tap.h).

The protocol the hooker relies on is that of diffusers' ``JointAttnProcessor2_0`` on ``pipe.transformer.transformer_blocks[*].attn``:

    attn.heads, attn.scale, attn.processor, attn.set_processor(p)
    processor(attn, hidden_states, encoder_hidden_states=None, attention_mask=None, ...)
    q     = attn.norm_q(attn.to_q(hidden_states))                      image queries
    k_img = attn.norm_k(attn.to_k(hidden_states))                      image keys
    k_txt = attn.norm_added_k(attn.add_k_proj(encoder_hidden_states))  text keys

each norm acting on the head dim of ``[batch, rows, heads, d]`` and skipped where the attribute is ``None``.  The grid comes from
``pipe.transformer.config.sample_size`` / ``.patch_size`` and ``pipe.vae_scale_factor``; the prompt from ``pipe.check_inputs``.
``trace()`` and the UNet path are untouched by this module; nothing is located or allocated unless ``trace_joint`` is used.
"""
from __future__ import annotations

from typing import Any, List, Optional, Union

import torch

from . import engine as _engine
from .heatmap import GlobalHeatMap, SelfAffinity
from .hook import AggregateHooker, ModuleLocator, ObjectHooker

__all__ = ['trace_joint', 'JointHeatMapHooker', 'MMDiTJointAttentionLocator']

CLIP_ROWS = 77                                      # the CLIP rows come first in SD3's context; T5 rows follow


class MMDiTJointAttentionLocator(ModuleLocator[Any]):
    """``transformer.transformer_blocks[*].attn``, in block order."""

    def locate(self, model) -> List[Any]:
        return [block.attn for block in model.transformer_blocks]


def _transformer_dtype(transformer) -> Optional[torch.dtype]:
    dtype = getattr(transformer, 'dtype', None)
    if isinstance(dtype, torch.dtype):
        return dtype
    try:
        return next(transformer.parameters()).dtype
    except (AttributeError, StopIteration, TypeError):
        return None


def _head_dim(attn) -> int:
    inner = getattr(attn.to_q, 'out_features', None) or getattr(attn, 'inner_dim')
    return int(inner) // int(attn.heads)


def _self_affinity_of(affinity: Optional[_engine.JointAffinityState], who: str) -> SelfAffinity:
    """``compute_self_affinity()`` of ``trace_joint`` and ``trace_flux``: a copy of the running sums as a ``SelfAffinity``."""
    if affinity is None:
        raise ValueError('the trace was built without self_affinity=True')
    if affinity.sums is None or not affinity.calls:
        raise RuntimeError(f'No affinity found. Did you forget to call `with {who}(..., self_affinity=True)` during generation?')
    return SelfAffinity(affinity.sums.clone(), affinity.grid, affinity.slices, affinity.calls)


class JointHeatMapHooker(AggregateHooker):
    """``with trace_joint(pipe) as tc: pipe(prompt); tc.compute_global_heat_map()``.

    Every joint-attention call of the located blocks that carries ``encoder_hidden_states``, no attention mask and as many image
    tokens as the grid has cells adds the text columns of the kept half of its batch (``x[B // 2:]``, the conditional half under
    classifier-free guidance; a batch of 1 whole) to one f32 ``[T, h w]`` tensor, T the context length (``per_head=True``: to one
    plane per head).  The generation itself is bit-identical to the untraced one.

    ``height`` / ``width``: the size of the generation in pixels where it is not the pipeline's default; the grid is
    ``size / (vae_scale_factor * patch_size)``.

    ``self_affinity=True``: every tapped call also adds the IMAGE columns of the same softmax to one f32
    ``[h w, h w]`` matrix, on the same stream, from the same Q and image K and the statistics the tap has just written;
    ``compute_self_affinity()`` returns it as a ``SelfAffinity``, and ``compute_global_heat_map().propagate(aff, n)`` applies as on a
    UNet trace.  One thing differs from the UNet: a row sums to ``slices`` MINUS the mass the cell gave to the text keys
    (``matrix()``, ``of()`` and ``propagate()`` divide by the row sum, so they hold as they are).  Without the option nothing of it is
    loaded or allocated.

    ``attend=True``: a tappable call whose module also has ``add_q_proj``, ``add_v_proj`` and ``to_v`` is COMPUTED by
    the hooker: Q, K and V are projected once for the whole batch, ``daam_joint_attend_forward`` gives the attention output of the
    image and the text rows and leaves the image rows' softmax statistics behind, and the text columns (and, with
    ``self_affinity=True``, the image columns) of the kept half are formed from those statistics: the attention is computed once
    instead of twice.  This REPLACES the block's processor with the SD3 protocol of diffusers' ``JointAttnProcessor2_0`` for those
    calls: a pipeline with a custom processor (IP-adapter and the like) should not use it, and the generation is no longer
    bit-identical to the untraced one -- it is the same attention with the softmax in f32.  Every other call (a mask, no context,
    another length, a missing projection) goes to the original processor, with the tap beside it where the predicate above holds.
    Without the option nothing of it is loaded, located or allocated."""

    def __init__(self, pipeline, per_head: bool = False, height: Optional[int] = None, width: Optional[int] = None,
                 self_affinity: bool = False, attend: bool = False):
        transformer = getattr(pipeline, 'transformer', None)
        if transformer is None or not hasattr(transformer, 'transformer_blocks'):
            raise ValueError('trace_joint needs a pipeline with a `transformer` of joint-attention blocks (SD3 class); '
                             'UNet pipelines are traced with `trace`')
        dtype = _transformer_dtype(transformer)
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f'trace_joint reads fp16 or bf16 Q and K: the pipeline\'s transformer is {dtype}')
        self.pipe = pipeline
        self.per_head = bool(per_head)
        config = transformer.config
        cell = int(pipeline.vae_scale_factor) * int(config.patch_size)
        default = int(config.sample_size) * int(pipeline.vae_scale_factor)
        height, width = int(height or default), int(width or default)
        if height % cell or width % cell:
            raise ValueError(f'a generation of {height} x {width} pixels is no whole number of {cell}-pixel cells')
        self.grid = (height // cell, width // cell)
        self.cells = self.grid[0] * self.grid[1]
        if not 1 <= self.cells <= _engine.MAX_JOINT_CELLS:
            raise ValueError(f'a grid of {self.grid[0]} x {self.grid[1]} cells: the joint tap takes 1..{_engine.MAX_JOINT_CELLS} cells')
        located = MMDiTJointAttentionLocator().locate(transformer)
        for attn in located:
            if _head_dim(attn) not in _engine.JOINT_HEAD_DIMS:
                raise ValueError(f'trace_joint: head dim {_head_dim(attn)}: one of {_engine.JOINT_HEAD_DIMS}')
        self.state: Optional[_engine.JointTapState] = None      # made by the first tapped call, which knows the context length
        self.affinity = _engine.JointAffinityState(*self.grid) if self_affinity else None
        self.attend = _engine.JointAttendState() if attend else None
        self.last_prompt: str = ''
        super().__init__([_JointPipelineHooker(pipeline, self)] + [JointAttentionHooker(attn, self) for attn in located])

    # -- fed by the hookers ----------------------------------------------------------------------------------------------------------
    def _begin_generation(self, prompt) -> None:
        self.last_prompt = prompt if isinstance(prompt, str) else prompt[0]
        if self.state is not None:
            self.state.reset()
        if self.affinity is not None:
            self.affinity.reset()

    def _tap(self, q, k_txt, k_img, heads: int, scale: float) -> None:
        if self.state is None or self.state.tokens != k_txt.shape[1]:
            self.state = _engine.JointTapState(self.grid[0], self.grid[1], k_txt.shape[1], self.per_head)
        self.state.tap(q, k_txt, k_img, heads, scale)
        if self.affinity is not None:
            self.affinity.tap(q, k_img, heads, scale, self.state.stats)

    def _attend(self, q_img, k_img, v_img, q_txt, k_txt, v_txt, heads: int, scale: float):
        """The fused route of a tappable call: the attention of the whole batch, then the planes of the kept half from its statistics."""
        out_img, out_txt, stats = self.attend.forward(q_img, k_img, v_img, q_txt, k_txt, v_txt, heads, scale)
        first = q_img.shape[0] // 2
        kept = stats[first * heads * _engine.pad128(self.cells):]
        if self.state is None or self.state.tokens != k_txt.shape[1]:
            self.state = _engine.JointTapState(self.grid[0], self.grid[1], k_txt.shape[1], self.per_head)
        self.state.tap_from_stats(q_img[first:], k_txt[first:], heads, scale, kept)
        if self.affinity is not None:
            self.affinity.tap(q_img[first:], k_img[first:], heads, scale, kept)
        return out_img, out_txt

    # -- results ---------------------------------------------------------------------------------------------------------------------
    def _sums(self) -> torch.Tensor:
        if self.state is None or self.state.sums is None or not self.state.calls:
            raise RuntimeError('No heat maps found. Did you forget to call `with trace_joint(...)` during generation?')
        return self.state.sums

    def raw_heat_maps(self) -> torch.Tensor:
        """The running sums of all T context rows (T5 rows included) as f32 ``[T, h, w]``: the sum over tapped calls and slices."""
        sums = self._sums()
        plane = sums.sum(dim=0) if self.per_head else sums.clone()
        return plane.view(-1, *self.grid)

    def compute_global_heat_map(self, prompt: Optional[str] = None) -> GlobalHeatMap:
        """The mean over tapped calls and slices of the CLIP rows (the first 77 of the context), f32 ``[77, h, w]``, as a
        ``GlobalHeatMap`` with the pipeline's tokenizer: ``compute_word_heat_map`` / ``segment`` / ... apply as on a UNet trace."""
        maps = self.raw_heat_maps()[:CLIP_ROWS] / float(self.state.slices)
        return GlobalHeatMap(self.pipe.tokenizer, self.last_prompt if prompt is None else prompt, maps.contiguous())

    def compute_head_heat_maps(self) -> torch.Tensor:
        """f32 ``[heads, T, h, w]`` (a trace built with ``per_head=True``): per head the mean over tapped calls and batch entries."""
        if not self.per_head:
            raise ValueError('the trace was built without per_head=True')
        sums = self._sums()
        return (sums / float(self.state.slices // self.state.heads)).view(sums.shape[0], sums.shape[1], *self.grid)

    def compute_self_affinity(self) -> SelfAffinity:
        """The image-to-image affinity of the last generation (a trace built with ``self_affinity=True``): the image columns of the
        joint softmax summed over every tapped call and slice (a copy: the next generation starts over)."""
        return _self_affinity_of(self.affinity, 'trace_joint')


class _JointPipelineHooker(ObjectHooker):
    """A ``pipe(prompt)`` call starts a new generation: the prompt is remembered, the next tapped call overwrites the sums."""

    def __init__(self, pipeline, parent: JointHeatMapHooker):
        super().__init__(pipeline)
        self.parent = parent

    def _hook_impl(self):
        self.monkey_patch('check_inputs', self._before_generation)

    def _before_generation(self, _pipe, *args, **kwargs):
        prompt: Union[str, List[str], None] = args[0] if args else kwargs.get('prompt')
        if prompt is not None and not isinstance(prompt, str) and len(prompt) > 1:
            raise ValueError('Only single prompt generation is supported for heat map computation.')
        self.parent._begin_generation(prompt if prompt is not None else '')
        return self.monkey_super('check_inputs', *args, **kwargs)


class JointAttentionHooker(ObjectHooker):
    """The processor installed on every located ``attn``.  Without ``attend=True`` the model's output is what the ORIGINAL processor
    returns for the original arguments, so the traced generation is bit-identical to the untraced one; beside it, under ``no_grad``, a
    call with ``encoder_hidden_states``, no attention mask and a query length equal to the grid's cell count is tapped (module
    docstring).  With ``attend=True`` such a call on a module that has ``add_q_proj``, ``add_v_proj`` and ``to_v`` does NOT reach the
    original processor: ``_attend`` computes it by the SD3 protocol with the attention from ``daam_joint_attend_forward``, and the
    generation is the same attention with the softmax in f32, no longer bit-identical (``JointHeatMapHooker``)."""

    def __init__(self, module, parent: JointHeatMapHooker):
        super().__init__(module)
        self.parent = parent

    def _hook_impl(self):
        self.original_processor = self.module.processor
        self.module.set_processor(self)

    def _unhook_impl(self):
        self.module.set_processor(self.original_processor)

    @staticmethod
    def _project(proj, norm, x, heads: int):
        y = proj(x)
        if norm is not None:
            batch, rows, channels = y.shape
            y = norm(y.view(batch, rows, heads, channels // heads)).reshape(batch, rows, channels)
        return y

    def _attend(self, attn, hidden_states, context):
        """``JointAttnProcessor2_0``'s protocol with the attention itself from ``daam_joint_attend_forward``: every projection once."""
        heads = attn.heads
        q_img = self._project(attn.to_q, getattr(attn, 'norm_q', None), hidden_states, heads)
        k_img = self._project(attn.to_k, getattr(attn, 'norm_k', None), hidden_states, heads)
        v_img = attn.to_v(hidden_states)
        q_txt = self._project(attn.add_q_proj, getattr(attn, 'norm_added_q', None), context, heads)
        k_txt = self._project(attn.add_k_proj, getattr(attn, 'norm_added_k', None), context, heads)
        v_txt = attn.add_v_proj(context)
        out_img, out_txt = self.parent._attend(q_img, k_img, v_img, q_txt, k_txt, v_txt, heads, attn.scale)
        out_img = attn.to_out[1](attn.to_out[0](out_img))
        if not getattr(attn, 'context_pre_only', False) and getattr(attn, 'to_add_out', None) is not None:
            out_txt = attn.to_add_out(out_txt)
        return out_img, out_txt

    def __call__(self, attn, hidden_states, *args, **kwargs):
        context = kwargs.get('encoder_hidden_states', args[0] if args else None)
        mask = kwargs.get('attention_mask', args[1] if len(args) > 1 else None)
        tappable = context is not None and mask is None and hidden_states.dim() == 3 and hidden_states.shape[1] == self.parent.cells
        if (tappable and self.parent.attend is not None
                and all(getattr(attn, name, None) is not None for name in ('add_q_proj', 'add_v_proj', 'to_v'))):
            with torch.no_grad():
                return self._attend(attn, hidden_states, context)
        out = self.original_processor(attn, hidden_states, *args, **kwargs)
        if tappable:
            with torch.no_grad():
                first = hidden_states.shape[0] // 2
                kept, ctx = hidden_states[first:], context[first:]
                heads = attn.heads
                q = self._project(attn.to_q, getattr(attn, 'norm_q', None), kept, heads)
                k_img = self._project(attn.to_k, getattr(attn, 'norm_k', None), kept, heads)
                k_txt = self._project(attn.add_k_proj, getattr(attn, 'norm_added_k', None), ctx, heads)
                self.parent._tap(q, k_txt, k_img, heads, attn.scale)
        return out


trace_joint = JointHeatMapHooker
