"""``trace`` / ``DiffusionHeatMapHooker``: the reference's tracing API (``daam/trace.py``)
over the MI355X-native extraction path.

Differences from the reference are confined to *how* the per-layer work is done:
  * the cross-attention processor does not materialise ``attention_probs`` on the default
    path: the attention itself runs on ``daam_attend`` (softmax(QK^T)V with the reference's
    rounding points, one MFMA kernel; the framework's fused SDPA where that kernel does not
    apply), and the heat-map tap either happens inside the same kernel (``defer_steps=0``) or
    recomputes the conditional-half probabilities from the projected Q / K in ONE launch for
    several denoising steps of all layers (``daam_tap_qk_enqueue`` / ``daam_tap_flush``, the default);
  * ``compute_global_heat_map`` is one fused bicubic + clamp + mean kernel.
The materialised path (``get_attention_scores`` -> ``daam_tap_probs`` -> ``bmm``) is kept for
``save_heads`` / ``load_heads``, attention masks, and ``tap='probs'``.
"""
from __future__ import annotations

import inspect
import math
import numbers
import os
import weakref
from pathlib import Path
from typing import Any, List, Optional, Type, Union

import torch
import torch.nn.functional as F

from .engine import HeatMapEngine, check_probes, check_time_bins, map_geometry, region_scores
from .coattention import KeyCoattention
from .heatmap import GlobalHeatMap, KeyScores, RawHeatMapCollection, RegionAttribution, Segmentation, SelfAffinity
from .hook import AggregateHooker, ObjectHooker, UNetCrossAttentionLocator, UNetSelfAttentionLocator
from .utils import cache_dir

__all__ = ['trace', 'DiffusionHeatMapHooker', 'GlobalHeatMap']


def _default_defer() -> int:
    return int(os.environ.get('DAAM_DEFER_STEPS', '64'))


def _default_defer_bytes(pipeline=None) -> int:
    """Bytes of recorded Q / K a trace may keep alive between tap launches: ``$DAAM_DEFER_BYTES``, else 40 % of the
    device memory that is free when the trace is set up (never less than 1 GiB, never more than 128 GiB; 32 GiB when the device
    cannot be asked).
    An MI355X has 288 GB: an SDXL-1024 generation holds 19.4 GB for its one launch, and SDXL at 2048 x 2048 (1.55 GB per
    denoising step, both CFG halves of every Q) gets the 64 steps a launch can take -- 100 steps = 2 launches, each
    re-reading the 0.88 GB of running sums once, instead of the 5 a fixed 32 GiB forced."""
    env = os.environ.get('DAAM_DEFER_BYTES')
    if env:
        return int(env)
    budget = 32 << 30
    try:
        dev = next(pipeline.unet.parameters()).device
        if dev.type != 'cuda' and torch.cuda.is_available():
            # cpu-offloaded pipelines keep their parameters on the host and run on the current device
            dev = torch.device('cuda', torch.cuda.current_device())
        if dev.type == 'cuda':
            free, _ = torch.cuda.mem_get_info(dev)
            # what torch's caching allocator holds but has not handed out is as good as free for the Q / K to come
            free += torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
            # absolute ceiling 128 GiB: enough for the 64 steps one launch takes at SDXL-2048 (99 GB), and it bounds what several
            # traces that each see the same free memory (ranks sharing a device) can pin between them
            budget = min(max(int(free * 0.4), 1 << 30), 128 << 30)
    except Exception:                                   # no parameters / no device yet: keep the default
        pass
    return budget


def _probe_embeddings(pipeline, probes, probe_embeds=None) -> torch.Tensor:
    """``[P, 77, C]`` conditional prompt embeddings of the probes: ``probe_embeds`` as given, else each probe encoded once by the
    pipeline's own ``encode_prompt`` (element ``[0]`` of what it returns: SD's 2-tuple and SDXL's 4-tuple both start with the
    conditional ``prompt_embeds``, SDXL's the concatenated 2048-wide embedding that ``attn2`` sees)."""
    if probe_embeds is not None:
        if not torch.is_tensor(probe_embeds) or probe_embeds.dim() != 3 or probe_embeds.shape[0] != len(probes) \
                or probe_embeds.shape[1] != 77:
            shape = list(probe_embeds.shape) if torch.is_tensor(probe_embeds) else type(probe_embeds).__name__
            raise ValueError(f'probe_embeds must be a [{len(probes)}, 77, C] tensor (one row set per probe), got {shape}')
        return probe_embeds
    encode = getattr(pipeline, 'encode_prompt', None)
    if encode is None:
        raise ValueError('the pipeline has no encode_prompt: pass probe_embeds')
    device = getattr(pipeline, '_execution_device', None) or getattr(pipeline, 'device', None)
    rows = []
    with torch.no_grad():
        for p in probes:
            out = encode(p, device=device, num_images_per_prompt=1, do_classifier_free_guidance=False)
            emb = out[0] if isinstance(out, (tuple, list)) else out
            if not torch.is_tensor(emb) or emb.dim() != 3 or emb.shape[0] != 1 or emb.shape[1] != 77:
                raise ValueError(f'encode_prompt({p!r}) gave no [1, 77, C] prompt embedding')
            rows.append(emb)
    return torch.cat(rows)


def _pipeline_dtype(pipeline) -> Optional[torch.dtype]:
    """The dtype of the pipeline's UNet (its ``dtype``, else that of its first parameter); ``None`` where it cannot be told."""
    dtype = getattr(pipeline.unet, 'dtype', None)
    if isinstance(dtype, torch.dtype):
        return dtype
    try:
        return next(pipeline.unet.parameters()).dtype
    except (AttributeError, StopIteration, TypeError):
        return None


def _no_maps(filtered: bool) -> RuntimeError:
    """What the engine's ``LookupError('no heat maps')`` means to the caller (the reference's two texts, trace.py:119-124)."""
    if filtered:
        return RuntimeError('No heat maps found for the given parameters.')
    return RuntimeError('No heat maps found. Did you forget to call `with trace(...)` during generation?')


class DiffusionHeatMapHooker(AggregateHooker):
    def __init__(self, pipeline, low_memory: bool = False, load_heads: bool = False, save_heads: bool = False,
                 data_dir: Optional[str] = None, *, accumulate: str = 'exact', tap: str = 'qk',
                 defer_steps: Optional[int] = None, batch_prompts: bool = False, time_bins=None, probes=None,
                 probe_embeds: Optional[torch.Tensor] = None, height: Optional[int] = None, width: Optional[int] = None,
                 self_affinity: bool = False):
        """Positional arguments as in the reference (trace.py:23-30).  Keyword-only extras:
        ``accumulate`` = ``'exact'`` (running sums in the pipeline dtype, like the reference) or
        ``'float32'``; ``tap`` = ``'qk'`` (fused, default) or ``'probs'`` (materialised
        probabilities, bit-identical adds); ``defer_steps`` = denoising steps tapped per launch
        (0 = one launch per layer call; default ``$DAAM_DEFER_STEPS`` or 64, the most one launch takes).
        The Q / K of the recorded steps are kept alive until their launch: at most ``$DAAM_DEFER_BYTES``
        (default: 40 % of the device memory free at set-up; a 50-step SDXL-1024 generation holds 19.4 GB -- both CFG
        halves of every Q -- and runs as ONE tap launch, issued when the maps are first read).
        ``batch_prompts=True`` accepts ``pipe([p0, ..., pN-1])`` (classifier-free guidance, any ``num_images_per_prompt``):
        ``compute_global_heat_maps`` then gives one map per prompt from one grouped finalize; ``False`` keeps the
        reference's single-prompt rule.
        ``time_bins`` (ints: the first denoising step of each window, starting at 0, strictly increasing, 1 to 64 of them) splits
        the running sums by time: window ``i`` holds the steps ``[time_bins[i], time_bins[i+1])``, the last one is open-ended.  A
        call's step is the number of tapped calls of its layer since the generation began.  ``compute_global_heat_map(time_bin=)``
        then selects a window or a range of them, ``compute_time_heat_maps`` gives one map per window; ``None`` keeps one sum
        over the whole generation (the reference's running sum, which the reference's unused ``time_idx`` never splits,
        trace.py:38,61-62).
        ``probes`` (1 to 8 prompt strings; open-vocabulary heat maps): every tapped call's conditional-half queries are also
        attended to the keys ``to_k(norm_cross(E_p))`` of each probe prompt -- with the generation's rounding points and sum dtype,
        never its attention mask -- into sums of their own; the generation itself is unchanged.  ``E_p`` is
        ``pipe.encode_prompt(p, device=..., num_images_per_prompt=1, do_classifier_free_guidance=False)[0]``, encoded once here;
        ``probe_embeds`` ([P, 77, C]) replaces that encoding (the strings still name the tokens).  ``compute_probe_heat_map(p)`` /
        ``compute_probe_heat_maps()`` / ``raw_probe_heat_maps(p)`` read them.  Each probe holds one more set of running sums (221 MB
        for SDXL-1024 with fp16 sums).  Not with ``time_bins``, ``save_heads`` or ``load_heads`` (ValueError).
        ``height`` / ``width`` (both or neither; ints): the pixel size that will be passed to ``pipe(...)``, for generations that are
        not the pipeline's default square -- SDXL at 832 x 1216 and the like.  The map is then ``out_h x out_w`` =
        ``height // cell x width // cell`` with ``cell`` = 8 px (SD) or 16 px (SDXL) (``engine.map_geometry``: both sizes multiples of
        ``2 * cell``, at most 128 cells per side), the running sums are ``[heads, 77, h, w]`` per layer (position ``p`` = pixel
        ``(p // w, p % w)``) and every ``compute_*_heat_map(s)`` returns ``[rows, out_h, out_w]`` maps.  A tapped layer whose size
        does not divide the map by its factor is a ValueError.  ``height == width ==`` the pipeline's default size is the default
        trace.  Not with ``time_bins`` (ValueError: the window-range reduction is not extended to such maps).
        ``self_affinity=True`` also taps the self-attention (``attn1``) of the transformer blocks whose ``attn2`` is tapped: every call
        whose query length is the cell count of the global heat map adds its head-summed ``softmax(Q K^T scale)`` (the kept half of the
        batch) into one f32 ``[h w, h w]`` matrix over all steps, which ``compute_self_affinity()`` returns as a ``SelfAffinity``
        (``GlobalHeatMap.propagate`` spreads word maps along it).  The model's own output still comes from the original
        processor with the original arguments.  Not with ``batch_prompts`` (ValueError: per-prompt affinities are out of scope),
        nor on a pipeline whose UNet is neither fp16 nor bf16 (ValueError here, not in the middle of a generation).
        ``False`` locates nothing, installs nothing and allocates nothing."""
        if tap not in ('qk', 'probs'):
            raise ValueError("tap must be 'qk' or 'probs'")
        if self_affinity and batch_prompts:
            raise ValueError('self_affinity cannot be combined with batch_prompts (one affinity per prompt is out of scope)')
        if self_affinity and _pipeline_dtype(pipeline) not in (None, torch.float16, torch.bfloat16):
            raise ValueError(f'self_affinity reads fp16 or bf16 Q and K: the pipeline\'s UNet is {_pipeline_dtype(pipeline)}')
        self.probes = check_probes(probes, time_bins)
        self.time_bins = check_time_bins(time_bins)
        if self.probes is not None and (save_heads or load_heads):
            raise ValueError('probes cannot be combined with save_heads / load_heads')
        self.probe_embeds = None if self.probes is None else _probe_embeddings(pipeline, self.probes, probe_embeds)
        if self.probes is None and probe_embeds is not None:
            raise ValueError('probe_embeds needs probes (the strings that name its tokens)')
        h = pipeline.unet.config.sample_size * pipeline.vae_scale_factor
        self.latent_hw = 4096 if h == 512 or h == 1024 else 9216          # trace.py:32-33
        out_hw = None
        if height is not None or width is not None:
            if height is None or width is None:
                raise ValueError('height and width go together: pass both (the size given to pipe(...)) or neither')
            if time_bins is not None:
                raise ValueError('time_bins cannot be combined with height / width')
            out_hw = map_geometry(h, height, width)
            if out_hw[0] * out_hw[1] == self.latent_hw and out_hw[0] == out_hw[1]:
                out_hw = None                                              # the pipeline's default size: the default trace
            else:
                self.latent_hw = out_hw[0] * out_hw[1]                     # trace.py:285 takes the factor from it
        locate_middle = load_heads or save_heads
        self.locator = UNetCrossAttentionLocator(restrict={0} if low_memory else None,
                                                 locate_middle_block=locate_middle)
        modules_found = self.locator.locate(pipeline.unet)
        self.engine = HeatMapEngine(max(1, len(modules_found)), tokens=77,
                                    out_side=int(math.sqrt(self.latent_hw)), out_hw=out_hw, accumulate=accumulate,
                                    defer_steps=_default_defer() if defer_steps is None else defer_steps,
                                    defer_bytes=_default_defer_bytes(pipeline), reuse_context=True, time_bins=self.time_bins,
                                    n_probes=len(self.probes) if self.probes is not None else 0, self_affinity=bool(self_affinity))
        self.all_heat_maps = RawHeatMapCollection(self.engine)
        self.last_prompt: str = ''
        self.last_prompts: List[str] = []
        self.last_image = None
        self.last_images: list = []
        self.batch_prompts = bool(batch_prompts)
        self._batch_unchecked = False                                      # the first tapped call of a generation validates its batch
        self._encode_args = None                                           # (num_images_per_prompt, do_classifier_free_guidance)
        self.time_idx = 0
        self._gen_idx = 0
        self.tap_mode = tap

        # the child hookers see this object through a weak proxy: no parent <-> child reference cycle, so a trace
        # that goes out of scope releases its context and running sums immediately
        me = weakref.proxy(self)
        hookers: List[ObjectHooker] = [
            UNetCrossAttentionHooker(m, me, layer_idx=idx, latent_hw=self.latent_hw, load_heads=load_heads,
                                     save_heads=save_heads, data_dir=data_dir)
            for idx, m in enumerate(modules_found)
        ]
        if self_affinity:
            self_locator = UNetSelfAttentionLocator(restrict={0} if low_memory else None, locate_middle_block=locate_middle)
            hookers += [UNetSelfAttentionHooker(m, me, cells=self.engine.out_h * self.engine.out_w)
                        for m in self_locator.locate(pipeline.unet)]
        hookers.append(PipelineHooker(pipeline, me))
        if type(pipeline).__name__ == 'StableDiffusionXLPipeline':           # trace.py:55-56
            hookers.append(ImageProcessorHooker(pipeline.image_processor, me))
        super().__init__(hookers)
        self.pipe = pipeline

    def time_callback(self, *args, **kwargs):
        self.time_idx += 1

    @property
    def layer_names(self):
        return self.locator.layer_names

    def _hook_impl(self):
        super()._hook_impl()
        # the installed processors / patched pipeline methods see the trace through weak proxies (no reference cycle
        # while idle); WHILE hooked they must keep it alive -- ``trace(pipe).hook()`` without holding on to the object is
        # legal with the reference -- so the hookers pin it until unhook() breaks the cycle again
        for member in self.module:
            member._pinned_trace = self

    def _unhook_impl(self):
        super()._unhook_impl()
        for member in self.module:
            member._pinned_trace = None
        self.engine.flush()

    def to_experiment(self, path, seed=None, id='.', subtype='.', prompt_idx: Optional[int] = None, **compute_kwargs):
        """trace.py:68-81.  ``prompt_idx`` (batched trace): export prompt ``prompt_idx`` -- its text, its map and its first image."""
        from .experiment import GenerationExperiment
        if prompt_idx is None:
            return GenerationExperiment(self.last_image, self.compute_global_heat_map(**compute_kwargs).heat_maps,
                                        self.last_prompt, seed=seed, id=id, subtype=subtype, path=path,
                                        tokenizer=self.pipe.tokenizer)
        prompt_idx = self._check_prompt_idx(prompt_idx)
        image = self.last_image
        n = len(self.last_prompts)
        if self.last_images and len(self.last_images) % n == 0:            # one image per sample: prompt p's first is p * k
            image = self.last_images[prompt_idx * (len(self.last_images) // n)]
        maps = self.compute_global_heat_map(prompt_idx=prompt_idx, **compute_kwargs).heat_maps
        return GenerationExperiment(image, maps, self.last_prompts[prompt_idx], seed=seed, id=id, subtype=subtype, path=path,
                                    tokenizer=self.pipe.tokenizer)

    # -- from the engine's maps to GlobalHeatMap -------------------------------------------------------
    def _n_rows(self, text: str) -> int:
        return len(self.pipe.tokenizer.tokenize(text)) + 2                 # 1 for SOS and 1 for padding (trace.py:127)

    def _wrap(self, maps: torch.Tensor, rows: int, text: str, normalize: bool) -> GlobalHeatMap:
        """``maps`` [>= rows, h, w] of the engine, cropped to the rows of ``text`` (a view), normalised in place on request."""
        maps = maps[:rows]
        if normalize:
            maps = self.engine.normalize_(maps)
        return GlobalHeatMap(self.pipe.tokenizer, text, maps)

    # -- time windows ------------------------------------------------------------------------------
    @property
    def n_time_bins(self) -> int:
        bins = getattr(self, 'time_bins', None)
        return len(bins) if bins is not None else 1

    def _bin_range(self, time_bin):
        """``time_bin`` -> ``(first, end)`` window range, or ``None`` (the whole generation).  An int (negative counts from the
        end) is one window; a slice with step ``None`` / 1 is a range, which must not be empty."""
        if time_bin is None:
            return None
        n = self.n_time_bins
        if isinstance(time_bin, slice):
            if time_bin.step not in (None, 1):
                raise ValueError(f'time_bin slice step must be None or 1, got {time_bin.step!r}')
            try:
                b0, b1, _ = time_bin.indices(n)
            except TypeError:
                raise ValueError(f'time_bin slice bounds must be ints: {time_bin!r}') from None
            if b0 >= b1:
                raise ValueError(f'time_bin {time_bin!r} selects no window of {n}')
            return b0, b1
        if isinstance(time_bin, bool) or not isinstance(time_bin, numbers.Integral):
            raise ValueError(f'time_bin must be an int, a slice or None, got {time_bin!r}')
        i = int(time_bin)
        if not -n <= i < n:
            raise ValueError(f'time_bin {i} out of range: the trace has {n} time window(s)')
        i %= n
        return i, i + 1

    def _check_bin_steps(self, rng) -> None:
        """A selected window range that received no step: RuntimeError naming the windows."""
        if rng is None or self.n_time_bins == 1:
            return
        steps = self.time_bin_steps()
        if not any(steps[rng[0]:rng[1]]):
            names = ', '.join(str(b) for b in range(*rng))
            raise RuntimeError(f'time window(s) {names} received no denoising steps in the last generation '
                               f'(steps per window: {steps})')

    def time_bin_steps(self) -> List[int]:
        """How many denoising steps each time window received in the last generation (one entry without ``time_bins``)."""
        return self.engine.window_steps()

    def raw_heat_maps(self, time_bin: int) -> dict:
        """``{(factor, layer, head): running sum [77, h, w]}`` of one time window: zero-copy views of the live sums, like
        ``all_heat_maps`` (which a trace with ``time_bins`` does not offer: it holds one sum per window)."""
        if isinstance(time_bin, slice):
            raise ValueError('raw_heat_maps takes one window (an int)')
        b0, _ = self._bin_range(time_bin)
        if self.engine.time_bins is None:
            return dict(self.engine.items())
        return self.engine.window_items(b0)

    def compute_time_heat_maps(self, prompt=None, factors=None, head_idx=None, layer_idx=None, normalize=False,
                               prompt_idx: Optional[int] = None) -> list:
        """One ``GlobalHeatMap`` per time window, from ONE grouped finalize per class (``daam_finalize_bins``; groups = windows,
        or windows x prompts; 64 groups per call).  The entry of a window that received no step is ``None``.  After a batched
        generation of N > 1 prompts, ``prompt_idx`` picks the prompt; without it each entry is the list of the N prompts' maps."""
        n = len(self.last_prompts)
        if prompt_idx is not None:
            prompt_idx = self._check_prompt_idx(prompt_idx)
        batched = n > 1
        if batched:
            prompts = list(self.last_prompts)
            if prompt is not None:
                prompts[prompt_idx if prompt_idx is not None else 0] = prompt
        else:
            prompts = [self.last_prompt if prompt is None else prompt]
        if self.engine.time_bins is None:                                  # one window: the whole generation
            if batched and prompt_idx is None:
                return [self.compute_global_heat_maps(factors, head_idx, layer_idx, normalize, prompts=prompts)]
            return [self.compute_global_heat_map(prompt, factors, head_idx, layer_idx, normalize, prompt_idx=prompt_idx)]
        steps = self.time_bin_steps()
        windows = [w for w, k in enumerate(steps) if k > 0]
        if not windows:
            raise _no_maps(False)
        n_rows = [self._n_rows(p) for p in prompts]
        which = [prompt_idx] if (batched and prompt_idx is not None) else list(range(len(prompts)))
        groups = [(w, w + 1, p) for w in windows for p in which]
        try:
            maps = self.engine.time_heat_maps(groups, len(prompts), n_rows, factors=factors, head_idx=head_idx,
                                              layer_idx=layer_idx)
        except LookupError:
            raise _no_maps(True) from None
        out: list = [None] * len(steps)
        for gi, (w, _, p) in enumerate(groups):
            hm = self._wrap(maps[gi], n_rows[p], prompts[p], normalize)
            if batched and prompt_idx is None:
                if out[w] is None:
                    out[w] = []
                out[w].append(hm)
            else:
                out[w] = hm
        return out

    # -- batched prompts ---------------------------------------------------------------------------
    def _check_prompt_idx(self, prompt_idx: int) -> int:
        n = len(self.last_prompts)
        if not isinstance(prompt_idx, int) or not 0 <= prompt_idx < max(n, 1):
            raise ValueError(f'prompt_idx {prompt_idx!r} out of range: the last generation traced {n} prompt(s)')
        return prompt_idx

    def _check_batch(self, batch: int):
        """First tapped call of a batched generation: the batch must be [uncond x N*k ; cond x N*k]."""
        self._batch_unchecked = False
        n = len(self.last_prompts)
        if n <= 1:                     # one prompt: any batch, with or without guidance, exactly as the default trace
            return
        if self._encode_args is not None:
            k, cfg = self._encode_args
            if not cfg:
                raise ValueError(f'{n} prompts traced without classifier-free guidance: per-prompt heat maps need the '
                                 f'[uncond ; cond] batch layout (the kept second half would split the prompts)')
            if k is not None and batch != 2 * n * int(k):
                raise ValueError(f'batch {batch} is not 2 x {n} prompts x {k} images per prompt (classifier-free guidance layout)')
        if batch % (2 * n):
            raise ValueError(f'batch {batch} does not divide into {n} prompt(s) under classifier-free guidance '
                             f'([uncond x N*k ; cond x N*k] needs a multiple of 2 x {n})')

    def compute_global_heat_maps(self, factors=None, head_idx=None, layer_idx=None, normalize=False,
                                 prompts: Optional[List[str]] = None, time_bin=None) -> List[GlobalHeatMap]:
        """One ``GlobalHeatMap`` per prompt of the last (batched) generation, each cropped to its own
        ``len(tokenize(p)) + 2`` rows, from ONE grouped finalize (``daam_finalize_groups``); the maps are views of one
        ``[N, 77, x, x]`` buffer.  Filters are per prompt: ``head_idx`` counts inside the prompt's keys.  ``prompts`` (one per
        traced prompt) replaces the texts that label and crop the maps, as ``prompt`` does in ``compute_global_heat_map``.
        ``time_bin``: the time window(s) to aggregate, as in ``compute_global_heat_map``."""
        rng = self._bin_range(time_bin)
        self._check_bin_steps(rng)
        if prompts is None:
            prompts = self.last_prompts or [self.last_prompt]
        elif len(prompts) != max(1, len(self.last_prompts)):
            raise ValueError(f'{len(prompts)} prompts given for {len(self.last_prompts)} traced')
        n_rows = [self._n_rows(p) for p in prompts]
        try:
            kw = {} if rng is None else dict(bins=rng)
            maps = self.engine.global_heat_maps(len(prompts), n_rows, factors=factors, head_idx=head_idx, layer_idx=layer_idx, **kw)
        except LookupError:
            raise _no_maps(head_idx is not None or layer_idx is not None) from None
        return [self._wrap(maps[p], rows, prompt, normalize) for p, (prompt, rows) in enumerate(zip(prompts, n_rows))]

    def compute_global_heat_map(self, prompt=None, factors=None, head_idx=None, layer_idx=None, normalize=False,
                                prompt_idx: Optional[int] = None, time_bin=None):
        """Aggregate over time (already summed by the tap), layers and heads (trace.py:83-132):
        per selected ``(factor, layer, head)`` key bicubic-resize the summed map to ``x*x``, clamp
        at 0, average the keys, keep ``len(tokenize(prompt)) + 2`` rows, optionally normalise per
        pixel over the content tokens.  Returns a ``GlobalHeatMap`` whose ``heat_maps`` is an
        fp32 device tensor.  After a batched generation of N > 1 prompts, ``prompt_idx`` picks the prompt
        (``compute_global_heat_maps`` gives all of them from one call).  ``time_bin`` (a trace with ``time_bins``): an int
        selects one time window, a slice a range of them (their sums are added per key before the bicubic and the clamp: the map
        of a generation that ran exactly those steps); ``None`` is the whole generation."""
        n = len(self.last_prompts)
        if prompt_idx is not None:
            prompt_idx = self._check_prompt_idx(prompt_idx)
        rng = self._bin_range(time_bin)
        if n > 1:
            if prompt_idx is None:
                raise ValueError(f'the last generation traced {n} prompts: pass prompt_idx, or use compute_global_heat_maps() '
                                 f'(a mean over every prompt\'s keys has no meaning)')
            prompts = list(self.last_prompts)
            if prompt is not None:
                prompts[prompt_idx] = prompt                              # labels AND crops, as on one prompt
            maps = self.compute_global_heat_maps(factors=factors, head_idx=head_idx, layer_idx=layer_idx, prompts=prompts,
                                                 time_bin=time_bin)[prompt_idx]
            if normalize:
                self.engine.normalize_(maps.heat_maps)
            return maps
        if prompt is None:
            prompt = self.last_prompt
        n_rows = self._n_rows(prompt)
        self._check_bin_steps(rng)
        try:
            # the crop is handed to the finalize: rows nobody reads are not computed (daam_finalize n_rows, ABI v6)
            kw = {} if rng is None else dict(bins=rng)
            maps = self.engine.global_heat_map(factors=factors, head_idx=head_idx, layer_idx=layer_idx, n_rows=n_rows, **kw)
        except LookupError:
            raise _no_maps(head_idx is not None or layer_idx is not None) from None
        return self._wrap(maps, n_rows, prompt, normalize)

    # -- self-attention affinity ---------------------------------------------------------------------------
    def compute_self_affinity(self) -> SelfAffinity:
        """The self-attention affinity of the last generation (a trace built with ``self_affinity=True``): a ``SelfAffinity`` over the
        grid of the global heat map, summed over every tapped ``attn1`` call of every step (a copy: the next generation starts over)."""
        state = self.engine.self_affinity
        if state is None:
            raise ValueError('the trace was built without self_affinity=True')
        if state.sums is None or state.calls == 0:
            h, w = state.grid
            raise RuntimeError(f'No self-attention maps found: no attn1 call of the last generation had {h} x {w} = {h * w} query positions. '
                               'Did you forget to call `with trace(..., self_affinity=True)` during generation?')
        return SelfAffinity(state.sums.clone(), state.grid, state.slices, state.calls)

    # -- head analysis -----------------------------------------------------------------------------------
    def compute_key_scores(self, regions=None, prompt=None, factors=None, head_idx=None, layer_idx=None,
                           prompt_idx: Optional[int] = None, time_bin=None) -> KeyScores:
        """Which heads and layers carry a word: for every selected ``(factor, layer, head)`` key the scores that
        ``compute_global_heat_map(head_idx=, layer_idx=).attribute(regions)`` gives for that key alone, from ONE device pass over the
        running sums (``HeatMapEngine.key_scores``) instead of one finalize per key.  ``regions``: ``None`` (one column: each token
        row's total clamped mass), a uint8 / bool mask or stack of masks at image resolution, a ``Segmentation`` (its masks), or a
        ``RegionAttribution`` (its footprint is reused).  Rows are cropped to ``len(tokenize(prompt)) + 2``; ``factors`` /
        ``head_idx`` / ``layer_idx`` / ``prompt_idx`` / ``time_bin`` mean what they mean in ``compute_global_heat_map`` and fail as
        they do there; non-square traces work.  Probes are out of scope: the scores are those of the generation's own prompt."""
        prompt, kw = self._key_selection(prompt, factors, head_idx, layer_idx, prompt_idx, time_bin)
        eng = self.engine
        area = footprint = None
        if isinstance(regions, RegionAttribution):
            area, footprint = regions.area, regions.footprint
        elif regions is not None:
            masks = regions.masks if isinstance(regions, Segmentation) else regions
            _, area, footprint = region_scores(None, masks, map_hw=(eng.out_h, eng.out_w))
        keys, scores = self._key_call(eng.key_scores, footprint, **kw)
        return KeyScores(keys, scores, area, list(self.layer_names), self.pipe.tokenizer, prompt)

    def compute_key_coattention(self, prompt=None, factors=None, head_idx=None, layer_idx=None, prompt_idx: Optional[int] = None,
                                time_bin=None) -> KeyCoattention:
        """Which heads and layers entangle two words: for every selected ``(factor, layer, head)`` key the Gram matrix of its token
        planes, from ONE device pass over the raw running sums (``HeatMapEngine.token_gram``; no bicubic, no clamp, no threshold).
        ``KeyCoattention.of('dog', 'cat')`` is then the cosine of the two word maps per key.  Rows are cropped to
        ``len(tokenize(prompt)) + 2``; every argument means what it means in ``compute_key_scores`` and fails as it fails there;
        batched prompts, time windows and non-square traces work.  Probes are out of scope."""
        prompt, kw = self._key_selection(prompt, factors, head_idx, layer_idx, prompt_idx, time_bin)
        keys, gram = self._key_call(self.engine.token_gram, **kw)
        return KeyCoattention(keys, gram, list(self.layer_names), self.pipe.tokenizer, prompt)

    def compute_key_heat_map(self, keys, weights=None, prompt=None, normalize=False, prompt_idx: Optional[int] = None,
                             time_bin=None) -> GlobalHeatMap:
        """The heat map of a chosen set of ``(factor, layer, head)`` keys: ``sum_k weights[k] * max(bicubic(sum_k), 0)`` over the
        listed keys, from ONE device pass (``HeatMapEngine.key_blend``) that reads only them.  ``keys``: a sequence of
        ``(factor, layer, head)`` -- the layer an index or a name of ``layer_names``, the head counted inside the prompt's block --
        or the ``[(key, score)]`` pairs ``KeyScores.top_keys`` / ``KeyCoattention.top_keys`` return.  ``weights=None`` is the mean
        over the listed keys (with every key listed: ``compute_global_heat_map()``); given weights are used as they are (negative
        ones subtract: heads A minus heads B), and a key listed twice adds its weights.  Rows are cropped, and ``normalize``,
        ``prompt``, ``prompt_idx`` and ``time_bin`` mean what they mean in ``compute_global_heat_map``; non-square traces work.
        ValueError for a key that was not tapped; probes are out of scope."""
        return self.compute_key_heat_maps([keys if weights is None else (keys, weights)], prompt=prompt, normalize=normalize,
                                          prompt_idx=prompt_idx, time_bin=time_bin)[0]

    def compute_key_heat_maps(self, selections, prompt=None, normalize=False, prompt_idx: Optional[int] = None,
                              time_bin=None) -> List[GlobalHeatMap]:
        """One ``GlobalHeatMap`` per entry of ``selections`` -- each ``keys`` or ``(keys, weights)`` as in ``compute_key_heat_map``
        -- from one pass over the union of their keys (8 selections per device call): a key no selection lists is not read, and
        every map is bit for bit the one ``compute_key_heat_map`` gives for its entry alone."""
        text, kw = self._key_selection(prompt, None, None, None, prompt_idx, time_bin)
        selections = [self._key_weights(entry) for entry in selections]
        if not selections or any(not keys for keys, _ in selections):
            raise _no_maps(True)
        eng = self.engine
        # the selection's key order without a device call: the descriptors are cached, the weights are not built yet
        try:
            rows, planes = eng._key_selection(**dict(kw, bins=kw.get('bins')))
            have, _ = eng._key_planes(*planes)
        except LookupError:
            raise _no_maps(False) from None
        column = {key: i for i, key in enumerate(have)}
        table = torch.zeros(len(selections), len(have), dtype=torch.float32)
        for g, (keys, weights) in enumerate(selections):
            for key, weight in zip(keys, weights):
                if isinstance(key[1], str):
                    # the reference's names restart per block (hook.py), so the factor and the head help to tell the layers apart
                    found = [i for i, name in enumerate(self.layer_names) if name == key[1] and (key[0], i, key[2]) in column]
                    if len(found) > 1:
                        raise ValueError(f'key {key!r}: layers {found} share that name and factor; pass the layer\'s index')
                    key = (key[0], found[0] if found else -1, key[2])
                if key not in column:
                    raise ValueError(f'key {key!r} was not tapped in the last generation')
                table[g, column[key]] += weight
        _, maps = self._key_call(eng.key_blend, table, **kw)
        return [self._wrap(maps[g], rows, text, normalize) for g in range(len(selections))]

    def _key_weights(self, entry):
        """An entry of ``compute_key_heat_maps`` -> ``([(factor, layer index or name, head)], [weight])``."""
        def is_key(x):
            return isinstance(x, (tuple, list)) and len(x) == 3 and isinstance(x[0], numbers.Number)

        def is_pair(x):                                                   # a (key, score) pair of top_keys
            return isinstance(x, (tuple, list)) and len(x) == 2 and is_key(x[0]) and isinstance(x[1], numbers.Number)

        keys, weights = entry, None
        if isinstance(entry, tuple) and len(entry) == 2 and not is_key(entry[0]) and not is_pair(entry[0]):
            keys, weights = entry
        out = []
        for key in keys:
            if is_pair(key):
                key = key[0]
            if not is_key(key):
                raise ValueError(f'key {key!r}: expected (factor, layer, head)')
            factor, layer, head = key
            if isinstance(layer, str):
                if layer not in self.layer_names:
                    raise ValueError(f'key {tuple(key)!r}: the pipeline has no layer named {layer!r}')
                out.append((int(factor), layer, int(head)))      # resolved against the tapped keys by the caller
            else:
                out.append((int(factor), int(layer), int(head)))
        if weights is None:
            weights = [1.0 / len(out)] * len(out) if out else []
        else:
            weights = [float(w) for w in (weights.tolist() if isinstance(weights, torch.Tensor) else weights)]
            if len(weights) != len(out):
                raise ValueError(f'{len(weights)} weights for {len(out)} keys')
        return out, weights

    def _key_selection(self, prompt, factors, head_idx, layer_idx, prompt_idx, time_bin):
        """What the per-key analyses decide before their engine call: ``(prompt, kw)`` -- the text that labels and crops the result,
        and the engine method's keywords: the crop, the filters, the prompt's block and the window range (``_key_call`` makes the
        call)."""
        n = len(self.last_prompts)
        if prompt_idx is not None:
            prompt_idx = self._check_prompt_idx(prompt_idx)
        rng = self._bin_range(time_bin)
        if n > 1 and prompt_idx is None:
            raise ValueError(f'the last generation traced {n} prompts: pass prompt_idx')
        if prompt is None:
            prompt = self.last_prompts[prompt_idx] if n > 1 else self.last_prompt
        n_rows = self._n_rows(prompt)
        self._check_bin_steps(rng)
        return prompt, dict(n_rows=n_rows, factors=factors, head_idx=head_idx, layer_idx=layer_idx, n_prompts=max(n, 1),
                            prompt=prompt_idx or 0, **({} if rng is None else dict(bins=rng)))

    @staticmethod
    def _key_call(method, *args, **kw):
        """An engine method of the per-key analyses, its LookupError turned into the trace's 'no heat maps' error."""
        try:
            return method(*args, **kw)
        except LookupError:
            raise _no_maps(kw['head_idx'] is not None or kw['layer_idx'] is not None) from None

    # -- probes (open-vocabulary heat maps) ----------------------------------------------------------
    def _check_probe(self, probe) -> int:
        n = len(self.probes) if self.probes is not None else 0
        if n == 0:
            raise ValueError('the trace has no probes: pass probes=[...] to trace()')
        if isinstance(probe, bool) or not isinstance(probe, numbers.Integral) or not -n <= int(probe) < n:
            raise ValueError(f'probe {probe!r} out of range: the trace has {n} probe(s)')
        return int(probe) % n

    def raw_probe_heat_maps(self, probe: int) -> dict:
        """``{(factor, layer, head): running sum [77, h, w]}`` of probe ``probe`` -- the layout of ``raw_heat_maps`` / ``all_heat_maps``,
        zero-copy views of the live sums."""
        return self.engine.probe_items(self._check_probe(probe))

    def _probe_maps(self, probes: List[int], factors, head_idx, layer_idx, normalize, prompt_idx):
        """``[probe][prompt] -> GlobalHeatMap`` for ``probes``, from one grouped finalize (groups = probes x prompts)."""
        n = max(1, len(self.last_prompts))
        if prompt_idx is not None:
            prompt_idx = self._check_prompt_idx(prompt_idx)
        texts = [self.probes[p] for p in probes]
        n_rows = [self._n_rows(t) for t in texts]
        try:
            maps = self.engine.probe_heat_maps(probes, n, n_rows, factors=factors, head_idx=head_idx, layer_idx=layer_idx)
        except LookupError:
            raise _no_maps(head_idx is not None or layer_idx is not None) from None
        which = range(n) if prompt_idx is None else [prompt_idx]
        return [[self._wrap(maps[i * n + j], rows, text, normalize) for j in which] for i, (text, rows) in enumerate(zip(texts, n_rows))]

    def compute_probe_heat_map(self, probe: int, factors=None, head_idx=None, layer_idx=None, normalize=False,
                               prompt_idx: Optional[int] = None) -> GlobalHeatMap:
        """The global heat map of probe ``probe`` over its own ``len(tokenize(probe)) + 2`` token rows: the generation's queries
        attended to the probe's keys, then the finalize of ``compute_global_heat_map`` (bicubic, clamp, mean over the selected keys;
        ``factors`` / ``head_idx`` / ``layer_idx`` / ``normalize`` as there).  After a batched generation of N > 1 prompts,
        ``prompt_idx`` picks the prompt whose queries are used."""
        p = self._check_probe(probe)
        if len(self.last_prompts) > 1 and prompt_idx is None:
            raise ValueError(f'the last generation traced {len(self.last_prompts)} prompts: pass prompt_idx')
        return self._probe_maps([p], factors, head_idx, layer_idx, normalize, prompt_idx)[0][0]

    def compute_probe_heat_maps(self, factors=None, head_idx=None, layer_idx=None, normalize=False,
                                prompt_idx: Optional[int] = None) -> list:
        """One ``GlobalHeatMap`` per probe from ONE grouped finalize (``daam_finalize_groups``, groups = probes x prompts).  After a
        batched generation of N > 1 prompts without ``prompt_idx``, each entry is the list of the N prompts' maps."""
        self._check_probe(0)
        maps = self._probe_maps(list(range(len(self.probes))), factors, head_idx, layer_idx, normalize, prompt_idx)
        if len(self.last_prompts) > 1 and prompt_idx is None:
            return maps
        return [row[0] for row in maps]


class _CallInterceptor(ObjectHooker):
    """Wraps methods of one pipeline-side object.  ``WRAPS`` lists ``(attribute, handler name, strict)``;
    a handler receives the patched object first and reaches the original through ``self.monkey_super``."""

    WRAPS = ()

    def __init__(self, target, parent_trace: 'trace'):
        super().__init__(target)
        self.parent_trace = parent_trace

    def _hook_impl(self):
        for attribute, handler, strict in self.WRAPS:
            self.monkey_patch(attribute, getattr(self, handler), strict=strict)


class ImageProcessorHooker(_CallInterceptor):
    """SDXL pipelines post-process through ``pipe.image_processor``: remember the first image it returns
    (reference trace.py:135-147)."""

    WRAPS = (('postprocess', '_after_postprocess', True),)

    def _after_postprocess(self, _processor, *args, **kwargs):
        images = self.monkey_super('postprocess', *args, **kwargs)
        self.parent_trace.last_image = images[0]
        self.parent_trace.last_images = list(images)
        return images


class PipelineHooker(_CallInterceptor):
    """What a ``pipe(prompt)`` call means for the trace (reference trace.py:150-186): exactly one prompt, the
    running sums start from zero, the prompt and the generated image are remembered."""

    WRAPS = (('run_safety_checker', '_after_safety_checker', False),      # absent in SDXL pipelines
             ('check_inputs', '_before_generation', True),
             ('encode_prompt', '_on_encode_prompt', False))                 # batched traces: images per prompt, CFG

    def __init__(self, pipeline, parent_trace: 'trace'):
        super().__init__(pipeline, parent_trace)
        self.heat_maps = parent_trace.all_heat_maps

    def _before_generation(self, _pipe, prompt: Union[str, List[str]], *args, **kwargs):
        single = isinstance(prompt, str)
        t = self.parent_trace
        if not single and len(prompt) > 1 and not t.batch_prompts:
            raise ValueError('Only single prompt generation is supported for heat map computation.')
        self.heat_maps.clear()                                             # RawHeatMapCollection.clear -> daam_reset
        t.last_prompt = prompt if single else prompt[0]
        t.last_prompts = [prompt] if single else list(prompt)
        t._batch_unchecked = t.batch_prompts
        t._encode_args = None
        return self.monkey_super('check_inputs', prompt, *args, **kwargs)

    def _on_encode_prompt(self, _pipe, *args, **kwargs):
        try:
            original = next(v for n, v in reversed(self._journal) if n == 'encode_prompt')
            bound = inspect.signature(original).bind_partial(*args, **kwargs).arguments
        except (TypeError, ValueError, StopIteration):
            bound = kwargs
        if 'do_classifier_free_guidance' in bound:
            self.parent_trace._encode_args = (bound.get('num_images_per_prompt'), bool(bound['do_classifier_free_guidance']))
        return self.monkey_super('encode_prompt', *args, **kwargs)

    def _after_safety_checker(self, pipe, image, *args, **kwargs):
        checked = self.monkey_super('run_safety_checker', image, *args, **kwargs)
        processor = getattr(pipe, 'image_processor', None)
        if not processor:
            pils = pipe.numpy_to_pil(checked[0])
        elif torch.is_tensor(checked[0]):
            pils = processor.postprocess(checked[0], output_type='pil')
        else:
            pils = processor.numpy_to_pil(checked[0])
        self.parent_trace.last_image = pils[-1]
        self.parent_trace.last_images = list(pils)
        return checked


class UNetCrossAttentionHooker(ObjectHooker):
    """The attention processor installed on every located ``attn2`` (diffusers attention-processor protocol;
    replaces the reference's processor, trace.py:252-311).

    Default route: the model's output comes from ``HeatMapEngine.attend`` (``daam_attend``; the framework's fused SDPA
    for calls that kernel does not take) and the heat-map tap gets the projected Q / K (fused into the same kernel on
    an immediate trace, ``HeatMapEngine.tap_qk`` otherwise -- nothing ``[BH, hw, 77]``-sized is ever materialised).  Materialised route
    (``get_attention_scores`` -> ``tap_probs`` -> ``bmm``) for attention masks, ``upcast_softmax``,
    ``save_heads`` / ``load_heads`` and ``tap='probs'``."""

    def __init__(self, module, parent_trace: 'trace', context_size: int = 77, layer_idx: int = 0,
                 latent_hw: int = 9216, load_heads: bool = False, save_heads: bool = False,
                 data_dir: Union[str, Path, None] = None):
        super().__init__(module)
        self.trace = parent_trace
        self.heat_maps = parent_trace.all_heat_maps
        self.layer_idx = layer_idx
        self.context_size = context_size
        self.latent_hw = latent_hw
        self.save_heads, self.load_heads = save_heads, load_heads
        self.data_dir = cache_dir() / 'heads' if data_dir is None else Path(data_dir)
        self.data_dir.mkdir(parents=True, exist_ok=True)                   # the reference creates it eagerly too (:217)
        self._factors = {}                                                 # positions -> factor

    # -- installation ----------------------------------------------------------------------------
    def _hook_impl(self):
        attn = self.module
        self.original_processor = attn.processor
        # per-generation constants of the default route
        self._heads, self._scale = attn.heads, attn.scale
        self._round_logits = not getattr(attn, 'upcast_attention', False)
        self._fusable = (self.trace.tap_mode == 'qk' and not self.save_heads and not self.load_heads
                         and not getattr(attn, 'upcast_softmax', False))
        self._tap_qk = self.trace.engine.tap_qk           # the C++ recorder's entry point on a deferred trace
        # attention itself on the library's kernel (fp16, 77 keys, head_dim a multiple of 8 up to 160), with the tap fused in on an immediate
        # trace; DAAM_NO_ATTEND=1 keeps the framework's fused SDPA for the model's output
        self._attend = None if os.environ.get('DAAM_NO_ATTEND') else self.trace.engine.attend
        # probes: the fused route gets its probe-tapping form here, once; without probes every call runs exactly as before
        self._probe_embeds = self.trace.probe_embeds
        self._probe_key_dtype = None
        if self._probe_embeds is not None:
            self._fused = self._fused_probes
        attn.set_processor(self)

    def _unhook_impl(self):
        self.module.set_processor(self.original_processor)
        self.__dict__.pop('_fused', None)

    def _ensure_probe_keys(self, attn, like: torch.Tensor) -> None:
        """The probes' keys of this layer, ``to_k(norm_cross(E_p))`` (batch = the probes), computed on the layer's first tapped call
        of the trace (again only if the pipeline's dtype changes)."""
        if self._probe_key_dtype is like.dtype:
            return
        emb = self._probe_embeds.to(device=like.device, dtype=like.dtype)
        with torch.no_grad():
            ctx = emb if attn.norm_cross is None else attn.norm_cross(emb)
            keys = attn.to_k(ctx)
        self.trace.engine.set_probe_keys(self.layer_idx, keys)
        self._probe_key_dtype = like.dtype

    def _fused_probes(self, attn, hidden_states, context):
        """``_fused`` on a trace with probes: the probe keys exist before the call is recorded; a deferred launch adds each probe's
        chain of the recorded calls itself, an immediate trace taps the probes right after the generation."""
        query, key, value = attn.to_q(hidden_states), attn.to_k(context), attn.to_v(context)
        self.trace._gen_idx += 1
        batch, positions, channels = query.shape
        factor = self._factor(positions)
        tapped = factor != 8 and key.shape[1] == self.context_size          # trace.py:289
        if tapped:
            if self.trace._batch_unchecked:
                self.trace._check_batch(batch)
            self._ensure_probe_keys(attn, key)
        engine = self.trace.engine
        out = None
        if self._attend is not None and key.shape[1] == self.context_size:
            out = self._attend(self.layer_idx, query, key, value, self._heads, self._scale, factor, self._round_logits, tapped)
        if out is None and tapped:
            self._tap_qk(self.layer_idx, query, key, self._heads, self._scale, factor, self._round_logits)
        if tapped and not engine.defer_steps:
            engine.tap_probes(self.layer_idx, query, self._heads, self._scale, factor, self._round_logits)
        if out is not None:
            return out
        heads = self._heads
        head_dim = channels // heads
        out = F.scaled_dot_product_attention(query.view(batch, -1, heads, head_dim).transpose(1, 2),
                                             key.view(batch, -1, heads, head_dim).transpose(1, 2),
                                             value.view(batch, -1, heads, head_dim).transpose(1, 2), scale=self._scale)
        return out.transpose(1, 2).reshape(batch, -1, channels)

    @property
    def num_heat_maps(self):
        return len(self.heat_maps)

    # -- heads cache (one file per processor call of the generation, reference :246-250) --------------
    def _heads_file(self) -> Path:
        return self.data_dir / f'{self.trace._gen_idx}.pt'

    def _save_attn(self, attn_slice: torch.Tensor):
        torch.save(attn_slice, self._heads_file())

    def _load_attn(self) -> torch.Tensor:
        return torch.load(self._heads_file())

    # -- the processor call ------------------------------------------------------------------------
    def _factor(self, positions: int) -> int:
        factor = self._factors.get(positions)
        if factor is None:
            factor = self._factors[positions] = int(math.sqrt(self.latent_hw // positions))   # trace.py:285
        return factor

    def _is_tapped(self, tokens: int, factor: int) -> bool:
        return tokens == self.context_size and factor != 8                 # trace.py:289

    def _fused(self, attn, hidden_states, context):
        """Default route.  Runs 60-70 times per denoising step: the attribute lookups that cannot change during
        a generation (heads, scale, the engine's recorder entry point) are resolved once in ``_hook_impl``."""
        query, key, value = attn.to_q(hidden_states), attn.to_k(context), attn.to_v(context)
        self.trace._gen_idx += 1
        batch, positions, channels = query.shape
        factor = self._factor(positions)
        tapped = factor != 8 and key.shape[1] == self.context_size          # trace.py:289
        if tapped and self.trace._batch_unchecked:
            self.trace._check_batch(batch)
        if self._attend is not None and key.shape[1] == self.context_size:
            out = self._attend(self.layer_idx, query, key, value, self._heads, self._scale, factor, self._round_logits, tapped)
            if out is not None:
                return out
        if tapped:
            self._tap_qk(self.layer_idx, query, key, self._heads, self._scale, factor, self._round_logits)
        heads = self._heads
        head_dim = channels // heads
        out = F.scaled_dot_product_attention(query.view(batch, -1, heads, head_dim).transpose(1, 2),
                                             key.view(batch, -1, heads, head_dim).transpose(1, 2),
                                             value.view(batch, -1, heads, head_dim).transpose(1, 2), scale=self._scale)
        return out.transpose(1, 2).reshape(batch, -1, channels)

    def _materialised(self, attn, hidden_states, context, attention_mask):
        raw_query = attn.to_q(hidden_states)
        query, key, value = (attn.head_to_batch_dim(t) for t in (raw_query, attn.to_k(context), attn.to_v(context)))
        probs = attn.get_attention_scores(query, key, attention_mask)
        if self.save_heads:
            self._save_attn(probs)
        elif self.load_heads:
            probs = self._load_attn()
        self.trace._gen_idx += 1
        factor = self._factor(probs.shape[1])
        if self._is_tapped(probs.shape[-1], factor):
            if self.trace._batch_unchecked:
                self.trace._check_batch(probs.shape[0] // attn.heads)
            self.trace.engine.tap_probs(self.layer_idx, probs, factor)
            if self._probe_embeds is not None:                             # the probes: daam_tap_qk on the same Q, no mask
                self._ensure_probe_keys(attn, raw_query)
                self.trace.engine.tap_probes(self.layer_idx, raw_query, attn.heads, attn.scale, factor,
                                             not getattr(attn, 'upcast_attention', False))
        return attn.batch_to_head_dim(torch.bmm(probs, value))

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, **_ignored):
        if encoder_hidden_states is None:
            context = hidden_states
        elif attn.norm_cross is None:
            context = encoder_hidden_states
        else:
            context = attn.norm_cross(encoder_hidden_states)
        if self._fusable and attention_mask is None:       # prepare_attention_mask(None, ...) is None: nothing to prepare
            mixed = self._fused(attn, hidden_states, context)
        else:
            batch, positions, _ = hidden_states.shape
            attention_mask = attn.prepare_attention_mask(attention_mask, positions, batch)
            mixed = self._materialised(attn, hidden_states, context, attention_mask)
        return attn.to_out[1](attn.to_out[0](mixed))                       # output projection, dropout


class UNetSelfAttentionHooker(ObjectHooker):
    """The processor installed on every located ``attn1`` of a trace with ``self_affinity=True``.  The model's output is what the
    ORIGINAL processor returns for the original arguments, so the traced generation is bit-identical to the untraced one.  Beside it,
    under ``no_grad``, a call whose query length is the cell count of the global heat map and that carries no attention mask gives
    ``to_q`` / ``to_k`` of the kept half of its batch (``x[B // 2:]``, as the cross-attention tap keeps it; a batch of 1 whole) to
    ``HeatMapEngine.self_affinity_tap``."""

    def __init__(self, module, parent_trace: 'trace', cells: int):
        super().__init__(module)
        self.trace = parent_trace
        self.cells = int(cells)

    def _hook_impl(self):
        self.original_processor = self.module.processor
        self.module.set_processor(self)

    def _unhook_impl(self):
        self.module.set_processor(self.original_processor)

    def __call__(self, attn, hidden_states, *args, **kwargs):
        out = self.original_processor(attn, hidden_states, *args, **kwargs)
        context = kwargs.get('encoder_hidden_states', args[0] if args else None)
        mask = kwargs.get('attention_mask', args[1] if len(args) > 1 else None)
        if context is None and mask is None and hidden_states.dim() == 3 and hidden_states.shape[1] == self.cells:
            with torch.no_grad():
                kept = hidden_states[hidden_states.shape[0] // 2:]
                self.trace.engine.self_affinity_tap(attn.to_q(kept), attn.to_k(kept), attn.heads, attn.scale)
        return out


trace: Type[DiffusionHeatMapHooker] = DiffusionHeatMapHooker
