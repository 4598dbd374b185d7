"""Device-side state of one trace: the per-(layer, head) running sums and the native context.

Python owns the memory (torch tensors, so ``all_heat_maps`` hands out zero-copy views and the
caching allocator sees it); ``libdaam_hip.so`` does all arithmetic.  Mirrors what the
reference keeps in ``RawHeatMapCollection`` (daam/heatmap.py:148-172) plus the bodies of
``UNetCrossAttentionHooker.__call__`` between scores and bmm (daam/trace.py:285-294) and
``compute_global_heat_map`` (daam/trace.py:103-130).
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import sys
import weakref
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as nat

Key = Tuple[int, int, int]   # (factor, layer, head) -- daam/heatmap.py:145


class CallShape:
    """What a layer's last validated ``tap_qk`` / ``attend`` call looked like, with the descriptor built for it -- the
    per-layer cache entry of the engine.  ``csrc/daam_fastpath.cpp`` mirrors it field by field in ``struct CallShape``
    (``Recorder.set_cache`` / ``set_attend_cache`` copy an entry across)."""
    __slots__ = ('q_shape', 'k_shape', 'dtype', 'heads', 'scale', 'round_logits', 'factor', 'desc_ref', 'desc', 'desc_addr',
                 'q_numel', 'k_numel', 'held_bytes')

    def __init__(self, query, key, heads, scale, round_logits, factor, desc):
        self.q_shape, self.k_shape, self.dtype = query.shape, key.shape, query.dtype
        self.heads, self.scale, self.round_logits, self.factor = heads, scale, round_logits, factor
        self.desc = desc                                       # DaamQKDesc / DaamAttendDesc (kept alive here), or None
        self.desc_ref = nat.byref(desc) if desc is not None else None
        self.desc_addr = ctypes.addressof(desc) if desc is not None else 0
        self.q_numel, self.k_numel = query.numel(), key.numel()
        self.held_bytes = (self.q_numel + self.k_numel) * query.element_size()   # what a recorded call keeps alive

    def same_call(self, query, key, heads, scale, round_logits, factor=None) -> bool:
        return (self.q_shape == query.shape and self.k_shape == key.shape and self.dtype is query.dtype
                and key.dtype is self.dtype and self.heads == heads and self.scale == scale
                and self.round_logits == round_logits and (factor is None or self.factor == factor))

# pipeline / running-sum dtypes the library knows (include/daam_hip.h).  fp16 runs on the MFMA kernels;
# bf16 and fp32 on the any-shape kernels with the same rounding points.
_DTYPE_CODE = {torch.float16: nat.DAAM_F16, torch.float32: nat.DAAM_F32, torch.bfloat16: nat.DAAM_BF16}


def _contiguous_qk_desc(dtype, b, heads, hw, tokens, c, scale, round_logits, k_stride_b=None) -> 'nat.QKDesc':
    """``DaamQKDesc`` of contiguous ``query`` [b, hw, c] / ``key`` [b, tokens, c] straight out of the projections (``c`` =
    ``heads * head_dim``).  ``k_stride_b=0``: one key set serves every batch entry (the probes)."""
    d = c // heads
    return nat.QKDesc(in_dtype=_DTYPE_CODE[dtype], batch=b, heads=heads, hw=hw, tokens=tokens, head_dim=d,
                      round_logits=1 if round_logits else 0, scale=float(scale),
                      q_stride_b=hw * c, q_stride_h=d, q_stride_p=c,
                      k_stride_b=tokens * c if k_stride_b is None else k_stride_b, k_stride_h=d, k_stride_t=c)


# Parked native contexts (with their running-sum buffers) of closed engines, per (device, layers, tokens, map side,
# sum dtype).  A pipeline is usually traced once per generation: re-adopting the previous trace's context saves the
# 1.5 ms of set-up / tear-down and the device synchronisation that destroying a context implies (hipFree).
_PARKED: Dict[tuple, list] = {}
_PARK_LIMIT = 2


_FASTPATH_READY = False


def _load_fastpath():
    """The C++ recorder, or None when the extension is not built.  Its release thread (the storages of the recorded
    Q / K go back to the caching allocator off the interpreter's thread) is drained and stopped at interpreter exit,
    while torch is still intact; ``DAAM_SYNC_RELEASE=1`` frees inline instead."""
    global _FASTPATH_READY
    try:
        from . import _fastpath
    except ImportError:
        return None
    if not _FASTPATH_READY:
        import atexit
        atexit.register(_fastpath.shutdown)
        if os.environ.get('DAAM_SYNC_RELEASE'):
            _fastpath.set_sync_release(True)
        _FASTPATH_READY = True
    return _fastpath


def drain_released() -> None:
    """Block until every Q / K block released by a finished launch is back in the caching allocator (they are freed on
    a helper thread).  Only memory accounting needs this (``torch.cuda.memory_allocated`` right after a trace)."""
    fp = _load_fastpath()
    if fp is not None:
        fp.drain()


MAX_TIME_BINS = 64
MAX_MAP_SIDE = 128                                            # daam_ctx_create's limit per output side


def map_geometry(base: int, height: int, width: int) -> Tuple[int, int]:
    """``(out_h, out_w)``: the heat-map size of a generation of ``height x width`` pixels on a pipeline whose default size is
    ``base = unet.config.sample_size * vae_scale_factor``.  The reference fixes a square map of side ``x`` = 64 for 512 / 1024
    pipelines, else 96 (trace.py:32-33): one map cell is ``cell = base // x`` pixels (8 for SD, 16 for SDXL), and a
    generation of another size has ``height // cell x width // cell`` cells.  Both sizes must be multiples of ``2 * cell`` (the
    factor-2 layers stay integral) and give at most 128 cells per side; otherwise ValueError."""
    for name, v in (('base', base), ('height', height), ('width', width)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
            raise ValueError(f'{name} must be a positive int, got {v!r}')
    base, height, width = int(base), int(height), int(width)
    x = 64 if base in (512, 1024) else 96
    cell = base // x
    if cell <= 0:
        raise ValueError(f'pipeline size {base} is smaller than its {x} map cells')
    if height % (2 * cell) or width % (2 * cell):
        raise ValueError(f'height {height} and width {width} must be multiples of {2 * cell} (map cell {cell} px, pipeline size {base})')
    out_h, out_w = height // cell, width // cell
    if out_h > MAX_MAP_SIDE or out_w > MAX_MAP_SIDE:
        raise ValueError(f'{height} x {width} px gives a {out_h} x {out_w} map: at most {MAX_MAP_SIDE} cells per side')
    return out_h, out_w


def layer_geometry(out_h: int, out_w: int, positions: int) -> Tuple[int, int, int]:
    """``(factor, h, w)`` of a tapped call with ``positions`` query positions on an ``out_h x out_w`` map:
    ``factor = int(sqrt(out_h * out_w // positions))`` (trace.py:285 with ``latent_hw = out_h * out_w``), ``h = out_h // factor``,
    ``w = out_w // factor``; position ``p`` is pixel ``(p // w, p % w)``.  A layer whose size does not divide that way (a UNet
    whose down-sampling rounds differently) is a ValueError, not a guess."""
    positions = int(positions)
    if positions <= 0:
        raise ValueError(f'{positions} query positions')
    factor = int(math.sqrt(out_h * out_w // positions))
    if factor <= 0 or out_h % factor or out_w % factor or (out_h // factor) * (out_w // factor) != positions:
        raise ValueError(f'a layer of {positions} query positions does not fit a {out_h} x {out_w} map: factor {factor} '
                         f'gives {out_h / max(factor, 1):g} x {out_w / max(factor, 1):g}')
    return factor, out_h // factor, out_w // factor


def check_time_bins(time_bins) -> Optional[Tuple[int, ...]]:
    """``time_bins`` of ``trace``: ``None`` (no windows), or the first denoising step of each window -- ints, starting at 0,
    strictly increasing, 1 to 64 of them (``daam_ctx_set_time_bins``).  Returns them as a tuple."""
    if time_bins is None:
        return None
    if isinstance(time_bins, (str, bytes)):
        raise ValueError('time_bins must be an iterable of ints (first step of each window)')
    try:
        bins = list(time_bins)
    except TypeError:
        raise ValueError('time_bins must be an iterable of ints (first step of each window)') from None
    if not 1 <= len(bins) <= MAX_TIME_BINS:
        raise ValueError(f'time_bins must hold 1 to {MAX_TIME_BINS} window starts, got {len(bins)}')
    for b in bins:
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)):
            raise ValueError(f'time_bins entries must be ints, got {b!r}')
    bins = [int(b) for b in bins]
    if bins[0] != 0:
        raise ValueError(f'time_bins must start at step 0, got {bins[0]}')
    if any(b <= a for a, b in zip(bins, bins[1:])):
        raise ValueError(f'time_bins must be strictly increasing: {bins}')
    return tuple(bins)


def window_steps(time_bins: Sequence[int], layer_steps: Sequence[int]) -> List[int]:
    """Steps each window received: a layer tapped n times put its steps ``[0, n)`` into the windows by their first steps; a
    window's count is the most any layer put there."""
    out = [0] * len(time_bins)
    for n in layer_steps:
        for w, first in enumerate(time_bins):
            end = time_bins[w + 1] if w + 1 < len(time_bins) else n
            out[w] = max(out[w], max(0, min(n, end) - first))
    return out


MAX_PROBES = 8


def check_probes(probes, time_bins=None) -> Optional[Tuple[str, ...]]:
    """``probes`` of ``trace``: ``None``, or 1 to 8 prompt strings whose keys the generation's queries are also tapped against.
    ``time_bins`` together with probes is not supported (ValueError)."""
    if probes is None:
        return None
    if isinstance(probes, (str, bytes)):
        raise ValueError('probes must be a list of prompt strings, not one string')
    try:
        out = list(probes)
    except TypeError:
        raise ValueError('probes must be a list of prompt strings') from None
    if not 1 <= len(out) <= MAX_PROBES:
        raise ValueError(f'probes must hold 1 to {MAX_PROBES} prompts, got {len(out)}')
    for p in out:
        if not isinstance(p, str):
            raise ValueError(f'probes entries must be strings, got {p!r}')
    if time_bins is not None:
        raise ValueError('probes cannot be combined with time_bins')
    return tuple(out)


def probe_key_groups(layout: Sequence[Tuple[int, int, int, int]], total: int, n_probes: int, n_prompts: int,
                     factors: Optional[Sequence[int]] = None, head_idx: Optional[int] = None,
                     layer_idx: Optional[int] = None) -> List[int]:
    """``daam_finalize_groups``' key -> group table of the probe sums: group ``p * n_prompts + i`` is probe ``p`` seen by the
    queries of prompt ``i``.  ``layout`` = ``(probe, generation layer, key offset of the probe's slot, kept heads)``; the keys of
    a probe slot group by prompt exactly as the generation's keys do (``prompt_key_groups``), and the filters mean what they mean
    there (``layer_idx`` names the generation's layer)."""
    groups = [-1] * total
    for p in range(n_probes):
        part = prompt_key_groups([(layer, off, factor, heads) for q, layer, off, factor, heads in layout if q == p], total,
                                 n_prompts, factors, head_idx, layer_idx)
        for k, g in enumerate(part):
            if g >= 0:
                groups[k] = p * n_prompts + g
    return groups


def release_parked_contexts() -> None:
    """Destroy every parked context now (frees their sum buffers too).  Not called at interpreter exit on purpose:
    process teardown reclaims them, and no HIP call has to run while the runtime is shutting down."""
    for states in _PARKED.values():
        for st in states:
            st['lib'].daam_ctx_destroy(st['ctx'])        # synchronises the device first
    _PARKED.clear()


class HeatMapEngine:
    def __init__(self, n_layers: int, tokens: int = 77, out_side: int = 64, accumulate: str = 'exact',
                 defer_steps: int = 0, defer_bytes: int = 32 << 30, reuse_context: bool = False, time_bins=None,
                 n_probes: int = 0, out_hw: Optional[Tuple[int, int]] = None, self_affinity: bool = False):
        """``accumulate``: ``'exact'`` keeps the running sums in the pipeline dtype like the
        reference (fp16 sums on an fp16 pipeline, heatmap.py:156); ``'float32'`` is the
        accuracy mode.  ``defer_steps`` > 0 records Q/K pointers and taps ``defer_steps``
        denoising steps of all layers in one launch (at most 64); the Q / K of the recorded steps stay
        alive until then, and a launch is forced at the next step boundary once they add up to
        ``defer_bytes`` (both CFG halves count: 388 MB per SDXL-1024 step).  ``reuse_context``: ``close()`` parks
        the native context and the sum buffers for the next engine of the same geometry instead of destroying them
        (what ``trace`` asks for: one trace per generation is the normal use).  ``time_bins``: first step of each time window
        (``check_time_bins``); every layer then keeps one running sum per window, ``[n_bins, heads, tokens, side, side]``.
        ``n_probes`` (0 to 8): every layer also keeps one running sum per probe, in the slot ``(1 + p) * n_layers + layer`` of the same
        context (``probe_slot``), fed by the layer's queries against the probe's keys (``set_probe_keys``); one deferred launch taps
        the generation and every probe.  Each probe costs one more set of sums (221 MB for SDXL-1024 with fp16 sums) and records no
        Q / K of its own (``defer_bytes`` counts the generation's only).
        ``out_hw`` = ``(out_h, out_w)``: the map of a non-square generation (``map_geometry``; replaces ``out_side``).  Layers are then
        ``[heads, tokens, h, w]`` by ``layer_geometry``, maps ``[rows, out_h, out_w]``, and the finalize is ``finalize_rect_kernel``.
        Not with ``time_bins`` (ValueError); ``daam_finalize_prepare`` does not apply (the finalize clears its output itself).
        Equal sides are ``out_side``.
        ``self_affinity``: the engine also holds a ``SelfAffinityState`` on the map's grid, fed by ``self_affinity_tap``; it lives and
        dies with the engine (it is not parked with the context).  ``False`` holds nothing."""
        if accumulate not in ('exact', 'float32'):
            raise ValueError("accumulate must be 'exact' or 'float32'")
        self.lib = nat.load()
        self.n_layers = int(n_layers)
        self.tokens = int(tokens)
        self.out_side = int(out_side)
        if out_hw is not None:
            self.out_h, self.out_w = int(out_hw[0]), int(out_hw[1])
            if not (1 <= self.out_h <= MAX_MAP_SIDE and 1 <= self.out_w <= MAX_MAP_SIDE):
                raise ValueError(f'out_hw {out_hw!r}: 1 to {MAX_MAP_SIDE} cells per side')
            self.out_side = self.out_h                    # read only where the sides are equal
        else:
            self.out_h = self.out_w = self.out_side
        self.rect = self.out_h != self.out_w
        self.self_affinity: Optional['SelfAffinityState'] = SelfAffinityState(self.out_h, self.out_w) if self_affinity else None
        if self.rect and time_bins is not None:
            raise ValueError('time_bins cannot be combined with a non-square map (height= / width=)')
        self.accumulate = accumulate
        self.time_bins = check_time_bins(time_bins)
        self.n_bins = len(self.time_bins) if self.time_bins is not None else 0
        self.n_probes = int(n_probes)
        if not 0 <= self.n_probes <= MAX_PROBES:
            raise ValueError(f'n_probes must be 0 to {MAX_PROBES}, got {n_probes}')
        if self.n_probes and self.time_bins is not None:
            raise ValueError('probes cannot be combined with time_bins')
        self._probe_k: Dict[int, torch.Tensor] = {}      # layer -> [n_probes, tokens, C] probe keys (to_k output)
        self._probe_desc: Dict[bytes, 'nat.QKDesc'] = {}  # generation DaamQKDesc bytes -> the probes' descriptor (k_stride_b = 0)
        self.defer_steps = min(int(defer_steps), 64)     # the kernels stage at most 64 steps of pointers per launch
        self.defer_bytes = int(defer_bytes) if defer_bytes and defer_bytes > 0 else 1 << 62
        self.reuse_context = bool(reuse_context) and not os.environ.get('DAAM_NO_CTX_POOL')
        # debugging aid: remember tensor._version of every recorded Q / K and refuse to launch when one was written in
        # place between the processor call and the launch (deferred taps read them at launch time)
        self._check_versions = bool(os.environ.get('DAAM_CHECK_VERSIONS'))
        self._rec_stream: Optional[torch.cuda.Stream] = None   # stream the generation's Q / K are produced on
        self._views_out = False                           # all_heat_maps handed out views of the live sum buffers
        # slots whose buffers were kept across a reset: may hold an earlier generation's sums.  Read by window_items only; probe
        # slots land here too and are never looked at (probes and time_bins exclude each other)
        self._stale: set = set()
        self._held = 0                                    # bytes of recorded Q / K (Python recorder)
        self.ctx: Optional[nat.c_void_p] = None
        self.device: Optional[torch.device] = None
        self.acc_dtype: Optional[torch.dtype] = None
        self.acc: Dict[int, torch.Tensor] = {}           # layer -> [heads, tokens, side, side]
        self.layer_info: Dict[int, Tuple[int, int, int]] = {}   # layer -> (factor, heads, side)
        self.touched: List[int] = []                     # layers updated since clear(), first-update order
        # deferred taps: recorded per call (the tensors are kept alive until the flush)
        self._rec: List[tuple] = []                      # (layer, query, key, address of its DaamQKDesc)
        self._window = self.defer_steps                  # steps of one layer per launch
        self._cnt: List[int] = [0] * self.n_layers      # recorded steps per layer
        self._qk_cache: List[Optional[CallShape]] = [None] * self.n_layers
        self._att_cache: List[Optional[CallShape]] = [None] * self.n_layers   # attend(): per-layer call descriptors
        self._touched_flag: List[bool] = [False] * self.n_layers
        self._mask_cache: Dict[tuple, tuple] = {}        # finalize key tables per selection (_select)
        self._ks_cache: Dict[tuple, tuple] = {}          # key_scores: (keys, DaamKeyPlanes tensor) per selection and buffer addresses
        self._gram_scratch: Optional[torch.Tensor] = None    # token_gram: the partial matrices of keys of more than one chunk
        self._blend_scratch: Optional[torch.Tensor] = None   # key_blend: the partial maps of the chunks of keys
        # deferred mode: the per-call bookkeeping runs in the C++ recorder (csrc/daam_fastpath.cpp) when
        # that extension is built; the Python implementation below is the same logic and stays the
        # slow path (first call of a layer, shape changes) and the fallback.  Both only record host-side
        # pointers -- all arithmetic is in libdaam_hip either way.
        self._fast = None
        if self.defer_steps and not os.environ.get('DAAM_NO_FASTPATH') and not self._check_versions:
            _fastpath = _load_fastpath()
            if _fastpath is not None:
                # the recorder calls back into this engine through a weak reference: engine -> recorder is the
                # only strong edge, so dropping the trace frees the context and the running sums at once
                # (no reference cycle waiting for the garbage collector with 221 MB of sums attached)
                me = weakref.ref(self)
                self._fast = _fastpath.Recorder(self.n_layers,
                                                lambda *a, **k: me()._tap_qk_slow(*a, **k),
                                                lambda: me().flush(),
                                                lambda layer: me()._touch(layer))
                self._fast.set_window(self._window)
                self._fast.set_budget(self.defer_bytes)
                self.tap_qk = self._fast.tap
                # daam_attend from C++ too (the recorder gets the context and the entry point once the context exists)
                self._attend_addr = 0
                try:
                    self._attend_addr = ctypes.cast(self.lib.daam_attend, ctypes.c_void_p).value or 0
                except (ctypes.ArgumentError, TypeError, AttributeError):
                    pass                                   # not a ctypes library (tests drive the engine with a recording fake)
                self.attend = self._fast.attend
                self._sync_native()

    def _sync_native(self) -> None:
        """Tell the C++ recorder which native context (if any) its ``attend`` launches on."""
        if self._fast is not None:
            me = weakref.ref(self)
            ctx = self.ctx.value if self.ctx is not None and getattr(self.ctx, 'value', None) else 0
            self._fast.set_native(ctx or 0, self._attend_addr if ctx else 0, lambda *a, **k: HeatMapEngine.attend(me(), *a, **k))    # the Python method: the recorder's slow path

    # ---- lifetime --------------------------------------------------------------------------
    def _require_device(self, t: torch.Tensor) -> None:
        if t.device.type != 'cuda':
            raise RuntimeError(
                'daam_amd: heat-map extraction runs only on an MI355X (HIP device); got a tensor on '
                f'{t.device}. There is no CPU fallback.')
        if self.device is None:
            self.device = t.device
        elif self.device != t.device:
            raise RuntimeError(f'daam_amd: trace is bound to {self.device}, got a tensor on {t.device}')

    def _ensure_ctx(self, pipe_dtype: torch.dtype) -> None:
        if self.ctx is not None:
            return
        if pipe_dtype not in _DTYPE_CODE:
            raise RuntimeError(f'daam_amd: unsupported pipeline dtype {pipe_dtype} (fp16 / bf16 / fp32 only)')
        self.acc_dtype = torch.float32 if self.accumulate == 'float32' else pipe_dtype
        parked = _PARKED.get(self._park_key()) if self.reuse_context else None
        if parked:
            st = parked.pop()
            self.ctx, self.acc, self.layer_info = st['ctx'], st['acc'], st['layer_info']
            # whatever the previous owner queued (on its stream) comes first
            self._current_stream().wait_event(st['event'])
            nat.check(self.lib.daam_reset(self.ctx, self.stream))      # sums start from zero (lazily, like clear())
            self._stale = set(self.acc)
            self._sync_native()
            return
        ctx = nat.c_void_p()
        with torch.cuda.device(self.device):
            if self.rect:
                nat.check(self.lib.daam_ctx_create_rect(self.n_layers * (1 + self.n_probes), self.tokens, self.out_h, self.out_w,
                                                        _DTYPE_CODE[self.acc_dtype], nat.byref(ctx)))
            else:
                nat.check(self.lib.daam_ctx_create(self.n_layers * (1 + self.n_probes), self.tokens, self.out_side,
                                                   _DTYPE_CODE[self.acc_dtype],
                                                   nat.byref(ctx)))
        if self.time_bins is not None:
            try:
                nat.check(self.lib.daam_ctx_set_time_bins(ctx, self.n_bins, (ctypes.c_int32 * self.n_bins)(*self.time_bins)))
            except Exception:
                self.lib.daam_ctx_destroy(ctx)
                raise
        self.ctx = ctx
        self._sync_native()

    def _park_key(self) -> tuple:
        # DAAM_TAP_WALK is read when a native context is created: a context parked without the switch is not adopted with it
        walk = os.environ.get('DAAM_TAP_WALK', '')[:1] == '1'
        side = (self.out_h, self.out_w) if self.rect else self.out_side
        return (str(self.device), self.n_layers, self.tokens, side, self.acc_dtype, walk, self.time_bins, self.n_probes)

    def close(self) -> None:
        if self.ctx is not None:
            # a context whose sum buffers were handed out as views (all_heat_maps iteration) is not parked: the next
            # owner would overwrite what those views show.  Destroying the context leaves the (torch-owned) buffers
            # to the views.
            park = self.reuse_context and not self._views_out
            states = _PARKED.setdefault(self._park_key(), []) if park else None
            if states is not None and len(states) < _PARK_LIMIT:
                done = self._current_stream().record_event()
                states.append(dict(lib=self.lib, ctx=self.ctx, acc=self.acc, layer_info=self.layer_info, event=done))
                self.acc, self.layer_info = {}, {}
            else:
                self.lib.daam_ctx_destroy(self.ctx)
            self.ctx = None
            self._sync_native()
        self._forget_layers()
        self.touched.clear()
        self._touched_flag = [False] * self.n_layers
        self._drop_recorded()

    def _forget_layers(self) -> None:
        """No layer is configured any more: the sum buffers go (to whoever still holds them), and with them everything that was
        derived per layer -- the validated call shapes of both recorders and the finalize key tables."""
        self.acc, self.layer_info = {}, {}
        self._stale.clear()
        self._qk_cache = [None] * self.n_layers
        self._att_cache = [None] * self.n_layers
        self._mask_cache.clear()
        if self._fast is not None:
            self._fast.invalidate()

    def __del__(self):
        if sys is None or sys.is_finalizing():          # no HIP calls while the interpreter (and the HIP runtime) shut down
            return
        try:
            self.close()
        except Exception:
            pass

    def _current_stream(self) -> 'torch.cuda.Stream':
        return torch.cuda.current_stream(self.device)

    @property
    def stream(self) -> int:
        return self._current_stream().cuda_stream

    def _side(self, hw: int, factor: int):
        """A tapped call's layer size: ``int(sqrt(hw))`` (trace.py:233), or ``(h, w)`` on a non-square map (``layer_geometry``; the
        caller's factor must be the rule's)."""
        if not self.rect:
            return int(math.sqrt(hw))
        f, h, w = layer_geometry(self.out_h, self.out_w, hw)
        if f != factor:
            raise ValueError(f'a layer of {hw} query positions on a {self.out_h} x {self.out_w} map has factor {f}, the call says {factor}')
        return (h, w)

    def _ensure_layer(self, layer: int, heads: int, side, factor: int) -> None:
        """``side``: an int, or ``(h, w)`` (``_side``)."""
        info = self.layer_info.get(layer)
        if info == (factor, heads, side):
            return
        if info is not None:
            # the reference would simply start a new key set / fail on a shape mismatch in `+`
            self.flush()
        h, w = side if isinstance(side, tuple) else (side, side)
        shape = (heads, self.tokens, h, w) if self.time_bins is None else (self.n_bins, heads, self.tokens, h, w)
        for slot in [layer] + [self.probe_slot(p, layer) for p in range(self.n_probes)]:     # a probe's sums: the layer's geometry
            buf = torch.zeros(shape, dtype=self.acc_dtype, device=self.device)
            if isinstance(side, tuple):
                nat.check(self.lib.daam_layer_configure_rect(self.ctx, slot, heads, h, w, factor, buf.data_ptr()))
            else:
                nat.check(self.lib.daam_layer_configure(self.ctx, slot, heads, side, factor, buf.data_ptr()))
            self.acc[slot] = buf
            self._stale.discard(slot)
            self.layer_info[slot] = (factor, heads, side)
        self._mask_cache.clear()

    def probe_slot(self, probe: int, layer: int) -> int:
        """The context's layer slot that holds probe ``probe``'s sums of layer ``layer``."""
        return (1 + probe) * self.n_layers + layer

    def _touch(self, layer: int) -> None:
        if not self._touched_flag[layer]:
            if not self.touched:
                # first tap of a generation: this is the stream its Q / K are produced on (see flush)
                self._rec_stream = self._current_stream()
            self._touched_flag[layer] = True
            self.touched.append(layer)

    # ---- RawHeatMapCollection.clear (heatmap.py:170-172) -----------------------------------------
    def clear(self) -> None:
        self._drop_recorded()
        if self.self_affinity is not None:
            self.self_affinity.reset()
        self.touched.clear()
        self._touched_flag = [False] * self.n_layers
        self._set_window(self.defer_steps)
        if self._fast is not None:
            self._fast.reset_touched()
        if self.ctx is not None:
            nat.check(self.lib.daam_reset(self.ctx, self.stream))
            self._stale = set(self.acc)                    # kept buffers (unless the views take them, below): zeroed lazily
        if self._views_out:
            # the reference's clear() drops its dict and the tensors it handed out live on unchanged
            # (heatmap.py:170-172): leave the old buffers to those views and start the next generation on new ones.
            # The native context must forget them too -- daam_reset only marked them "to be zeroed", and a layer
            # that is not tapped again (another resolution turns its factor into 8) would otherwise be zeroed by the
            # next finalize: a write into memory the views own, or that is back in the caching allocator.
            if self.ctx is not None:
                for layer in list(self.layer_info):
                    nat.check(self.lib.daam_layer_release(self.ctx, layer))
            self._forget_layers()
            self._views_out = False

    # ---- tap -------------------------------------------------------------------------------------
    def self_affinity_tap(self, query: torch.Tensor, key: torch.Tensor, heads: int, scale: float) -> None:
        """One ``attn1`` call's ``to_q`` / ``to_k`` outputs ``[batch, h w, heads * d]`` (the kept half of the batch) into the affinity of
        an engine built with ``self_affinity=True``."""
        if self.self_affinity is None:
            raise ValueError('the engine was built without self_affinity=True')
        self.self_affinity.tap(query, key, heads, scale)

    def tap_qk(self, layer: int, query: torch.Tensor, key: torch.Tensor, heads: int, scale: float,
               factor: int, round_logits: bool = True) -> None:
        """``query`` [B, hw, heads*d], ``key`` [B, tokens, heads*d] straight out of ``to_q`` /
        ``to_k`` (trace.py:262,269); no ``head_to_batch_dim`` copy is made."""
        # Hot path (3000 calls per SDXL generation).  Full validation (shapes, dtypes, call parameters)
        # runs on a layer's first call of every launch window; inside a window only the invariants
        # that could silently change the memory layout are re-checked (element counts, dtype,
        # contiguity) -- every torch attribute access costs 50-100 ns here.
        c = self._qk_cache[layer]
        cnt = self._cnt
        if (c is None or cnt[layer] == 0 or not self.defer_steps):
            if (c is None or not c.same_call(query, key, heads, scale, round_logits, factor)
                    or not query.is_contiguous() or not key.is_contiguous()):
                query, key, c = self._prepare_qk(layer, query, key, heads, scale, factor, round_logits)
        elif (query.numel() != c.q_numel or key.numel() != c.k_numel or query.dtype is not c.dtype or c.scale != scale
              or not query.is_contiguous() or not key.is_contiguous()):
            query, key, c = self._prepare_qk(layer, query, key, heads, scale, factor, round_logits)
        if self.defer_steps:
            # record only: pointers cross the FFI in one daam_tap_qk_enqueue_many call per flush
            n = cnt[layer]
            if n >= self._window or (self._held >= self.defer_bytes and self._rec[0][0] == layer):
                self.flush()
                n = 0
            cnt[layer] = n + 1
            self._held += c.held_bytes
            if self._check_versions:
                self._rec.append((layer, query, key, c.desc_addr, query._version, key._version))
            else:
                self._rec.append((layer, query, key, c.desc_addr))
        else:
            rc = self.lib.daam_tap_qk(self.ctx, layer, query.data_ptr(), key.data_ptr(), c.desc_ref, self.stream)
            if rc:
                nat.check(rc)
        if not self._touched_flag[layer]:
            self._touch(layer)

    def _tap_qk_slow(self, layer: int, query: torch.Tensor, key: torch.Tensor, heads: int, scale: float,
                     factor: int, round_logits: bool = True) -> None:
        """Called by the C++ recorder for everything but the steady state: validates, rebuilds the
        layer's call descriptor, teaches the recorder the new call shape and records the tap."""
        f = self._fast
        c = self._qk_cache[layer] if 0 <= layer < self.n_layers else None
        fresh = (c is None or not c.same_call(query, key, heads, scale, round_logits, factor)
                 or not query.is_contiguous() or not key.is_contiguous())
        if fresh:
            query, key, c = self._prepare_qk(layer, query, key, heads, scale, factor, round_logits)
        if f.full(layer):
            self.flush()
        if fresh:
            f.set_cache(layer, query, key, int(heads), float(scale), int(factor), bool(round_logits), c.desc_addr)
        f.record(layer, query, key, c.desc_addr)
        self._touch(layer)

    @property
    def pending_taps(self) -> int:
        """Recorded taps that have not been launched yet."""
        return self._fast.count() if self._fast is not None else len(self._rec)

    def last_flush(self) -> dict:
        """Launch structure of the last deferred tap launch (``daam_last_flush``): kernels launched, how many of them ran on
        auxiliary streams beside the caller's, the longest per-layer step chain, and the number of tap launches this
        context has made so far."""
        if self.ctx is None:
            return dict(kernels=0, side_streams=0, max_steps=0, launches=0)
        k, sd, ms, n = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
        nat.check(self.lib.daam_last_flush(self.ctx, ctypes.byref(k), ctypes.byref(sd), ctypes.byref(ms), ctypes.byref(n)))
        return dict(kernels=k.value, side_streams=sd.value, max_steps=ms.value, launches=n.value)

    def last_kernels(self, which: int = 0) -> str:
        """Names of the kernel(s) the last tap launch (``which`` 0) / finalize call (1) really launched (``daam_last_kernels``)."""
        if self.ctx is None:
            return ''
        buf = ctypes.create_string_buffer(256)
        nat.check(self.lib.daam_last_kernels(self.ctx, which, buf, len(buf)))
        return buf.value.decode()

    def _pending(self, layer: int) -> int:
        return self._fast.pending(layer) if self._fast is not None else self._cnt[layer]

    def _set_window(self, w: int) -> None:
        self._window = w
        if self._fast is not None:
            self._fast.set_window(w)

    def _ensure_call_layer(self, layer: int, query: torch.Tensor, heads: int, factor: int) -> Tuple[int, int, int]:
        """Configure ``layer`` for a call whose ``query`` is [B, hw, heads*d]: the kept (conditional) half of ``B * heads`` planes
        of ``_side(hw, factor)``.  Returns ``query.shape``."""
        b, hw, c = query.shape
        bh = b * heads
        self._ensure_layer(layer, bh - bh // 2, self._side(hw, factor), factor)
        return b, hw, c

    def _prepare_qk(self, layer, query, key, heads, scale, factor, round_logits):
        """Slow path of ``tap_qk``: validate, (re)configure the layer, build the call descriptor.
        Returns ``(query, key, cache entry)`` with both tensors contiguous."""
        if not 0 <= layer < self.n_layers:
            raise IndexError(f'layer {layer} out of range (trace has {self.n_layers} layers)')
        self._require_device(query)
        query = query if query.is_contiguous() else query.contiguous()
        key = key if key.is_contiguous() else key.contiguous()
        self._ensure_ctx(query.dtype)
        if query.dtype != key.dtype:
            raise RuntimeError('daam_amd: query / key dtype mismatch')
        if query.dtype not in _DTYPE_CODE:
            raise RuntimeError(f'daam_amd: unsupported activation dtype {query.dtype} (fp16 / bf16 / fp32 only)')
        if self.acc_dtype not in (torch.float32, query.dtype):
            raise RuntimeError(f'daam_amd: {query.dtype} activations on a trace whose running sums are {self.acc_dtype} '
                               '(fp32 activations need fp32 sums; fp16 / bf16 sums need activations of the same dtype)')
        b, hw, c = self._ensure_call_layer(layer, query, heads, factor)
        desc = _contiguous_qk_desc(query.dtype, b, heads, hw, key.shape[1], c, scale, round_logits)
        # a shape change of a layer inside a deferred batch starts a new batch (the C side checks too)
        if self._pending(layer):
            self.flush()
        entry = CallShape(query, key, heads, scale, round_logits, factor, desc)
        self._qk_cache[layer] = entry
        return query, key, entry

    # ---- attend: the processor's attention on the library's kernel, tap fused in -------------------
    def attend(self, layer: int, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, heads: int, scale: float,
               factor: int, round_logits: bool = True, tapped: bool = True) -> Optional[torch.Tensor]:
        """``softmax(scale * Q K^T) V`` of one cross-attention call with the reference's rounding points
        (``get_attention_scores`` + ``bmm``, daam/trace.py:276,296-297) on ``daam_attend``; returns ``[B, hw, heads*d]``
        ready for the output projection, or ``None`` when the call is not one the kernel takes (not fp16 / bf16, head_dim not a
        multiple of 8 up to 160, not 77 keys, not contiguous): the caller then uses the framework's attention and ``tap_qk``.

        ``tapped``: the call passes the reference's gate (trace.py:289).  On an immediate trace (``defer_steps=0``) the
        heat-map update happens inside the same kernel; on a deferred trace the kernel only attends and Q / K are
        recorded for the batched launch, exactly as ``tap_qk`` would."""
        a = self._att_cache[layer] if 0 <= layer < self.n_layers else None
        if (a is None or a.q_shape != query.shape or a.k_shape != key.shape or a.dtype is not query.dtype or a.heads != heads
                or a.scale != scale or a.round_logits != round_logits):
            a = self._prepare_attend(layer, query, key, value, heads, scale, round_logits)
        if (a.desc is None or value.shape != a.k_shape or key.dtype is not a.dtype or value.dtype is not a.dtype
                or not (query.is_contiguous() and key.is_contiguous() and value.is_contiguous())
                or ((query.requires_grad or key.requires_grad or value.requires_grad) and torch.is_grad_enabled())):
            return None                                                    # the kernel has no backward: leave autograd to torch
        fused_tap = tapped and not self.defer_steps
        if fused_tap:
            c = self._qk_cache[layer]
            if c is None or not c.same_call(query, key, heads, scale, round_logits, factor):
                self._prepare_qk(layer, query, key, heads, scale, factor, round_logits)    # validates, configures the layer
        out = torch.empty_like(query)
        rc = self.lib.daam_attend(self.ctx, layer, query.data_ptr(), key.data_ptr(), value.data_ptr(), out.data_ptr(),
                                  a.desc_ref, 1 if fused_tap else 0, self.stream)
        if rc:
            if rc == nat.E_UNSUPPORTED:                    # e.g. a view whose data pointer is not 16-byte aligned
                return None
            nat.check(rc)
        if fused_tap:
            if not self._touched_flag[layer]:
                self._touch(layer)
        elif tapped:
            self.tap_qk(layer, query, key, heads, scale, factor, round_logits)
        return out

    def _prepare_attend(self, layer, query, key, value, heads, scale, round_logits):
        if not 0 <= layer < self.n_layers:
            raise IndexError(f'layer {layer} out of range (trace has {self.n_layers} layers)')
        self._require_device(query)
        desc = None
        d = query.shape[2] // heads if query.dim() == 3 and heads > 0 else 0
        # bf16 pipelines: the kernel rounds the logits to bf16 like the reference's baddbmm; upcast_attention (f32 logits) is left
        # to the framework's attention
        if ((query.dtype is torch.float16 or (query.dtype is torch.bfloat16 and round_logits))
                and query.dim() == 3 and key.dim() == 3 and key.shape[1] == self.tokens
                and d * heads == query.shape[2] and key.shape[2] == query.shape[2] and query.shape[0] == key.shape[0]
                and d % 8 == 0 and 8 <= d <= 160 and query.shape[1] % 8 == 0):
            self._ensure_ctx(query.dtype)
            if self.acc_dtype in (query.dtype, torch.float32):
                b, hw, c = query.shape
                qk = _contiguous_qk_desc(query.dtype, b, heads, hw, self.tokens, c, scale, round_logits)
                desc = nat.AttendDesc(qk=qk, v_stride_b=self.tokens * c, v_stride_h=d, v_stride_t=c,
                                      o_stride_b=hw * c, o_stride_h=d, o_stride_p=c)
        entry = CallShape(query, key, heads, scale, round_logits, 0, desc)
        self._att_cache[layer] = entry
        if self._fast is not None:
            self._fast.set_attend_cache(layer, query, key, int(heads), float(scale), bool(round_logits), entry.desc_addr)
        return entry

    def _launch_stream(self):
        """The stream a deferred launch goes to, ordered after the producers of the recorded Q / K: normally the
        current stream IS the stream they were produced on; when the maps are read from another stream (generation
        inside ``torch.cuda.stream(s)``, ``compute_global_heat_map`` outside), the launch waits for everything queued
        on the recording stream so far.  Returns ``(stream handle, recording stream or None)``."""
        cur = self._current_stream()
        rec = self._rec_stream
        if rec is None or rec.cuda_stream == cur.cuda_stream:
            return cur.cuda_stream, None
        cur.wait_stream(rec)
        return cur.cuda_stream, rec

    def flush(self, _before_launch=None) -> bool:
        """Run every recorded (deferred) tap; the held Q/K references are dropped afterwards
        (stream order keeps their memory valid until the kernel has consumed it).  ``_before_launch(stream)`` is called between
        handing the recorded calls to the library and the launch (``global_heat_map`` announces its output there, so that the
        launch's table-upload kernel clears it).  Returns whether anything was launched."""
        # the two recorders differ only in where the four arrays live; ``keep`` holds the Python recorder's until the call is made
        n, la, qa, ka, da, keep = (*self._fast.buffers(), None) if self._fast is not None else self._rec_buffers()
        if self.ctx is None or n == 0:
            return False
        try:
            stream, rec_stream = self._launch_stream()
            if self.n_probes:
                arrays = [np.ctypeslib.as_array((t * n).from_address(a)) for t, a in
                          ((ctypes.c_int32, la), (ctypes.c_uint64, qa), (ctypes.c_uint64, ka), (ctypes.c_uint64, da))]
                n, keep = self._with_probes(*arrays)
                la, qa, ka, da = (a.ctypes.data for a in keep)
            nat.check(self.lib.daam_tap_qk_enqueue_many(self.ctx, n, la, qa, ka, da))
            self._announce_then_launch(_before_launch, stream)
            if rec_stream is not None:
                # the Q / K blocks return to the recording stream's allocator pool: not before the tap has read them
                rec_stream.wait_stream(self._current_stream())
            self._set_window(self.defer_steps)
        finally:
            self._drop_recorded()
        return True

    def _rec_buffers(self):
        """The Python recorder's calls as the C++ recorder's ``buffers()`` gives its own: ``(n, layers, q, k, desc)``, the four as
        addresses of int32 / uint64 arrays, plus the arrays themselves (they must outlive the call).  ``n`` = 0 without a context."""
        rec = self._rec
        if self.ctx is None or not rec:
            return 0, 0, 0, 0, 0, None
        if self._check_versions:
            for layer, q, k, _d, qv, kv in rec:
                if q._version != qv or k._version != kv:
                    self._drop_recorded()
                    raise RuntimeError(f'daam_amd: the query / key of layer {layer} was modified in place between its '
                                       'attention call and the deferred tap launch (use defer_steps=0 for such a pipeline)')
            rec = [r[:4] for r in rec]
        lay_t, q_t, k_t, d_t = zip(*rec)                       # one C-level pass
        arrays = (np.array(lay_t, dtype=np.int32), np.array([t.data_ptr() for t in q_t], dtype=np.uint64),
                  np.array([t.data_ptr() for t in k_t], dtype=np.uint64), np.array(d_t, dtype=np.uint64))
        return (len(rec), *(a.ctypes.data for a in arrays), arrays)

    def _announce_then_launch(self, before_launch, stream) -> None:
        """The recorded calls are in the library's hands: whatever ``before_launch`` does, the launch that consumes (and drops) them
        must follow -- the Python references to their Q / K are released right after, and entries left pending would be read
        from freed memory by the next launch.  A failing announcement is re-raised after the launch."""
        failed = None
        if before_launch is not None:
            try:
                before_launch(stream)
            except BaseException as e:                         # noqa: BLE001 -- re-raised below
                failed = e
        rc = self.lib.daam_tap_flush(self.ctx, stream)
        if failed is not None:
            raise failed
        nat.check(rc)

    def _drop_recorded(self) -> None:
        self._rec.clear()
        self._held = 0
        self._cnt[:] = [0] * self.n_layers              # in place: tap_qk holds a reference across flush()
        if self._fast is not None:
            self._fast.drop()

    # ---- probes: the generation's queries against the keys of other prompts -------------------------
    def set_probe_keys(self, layer: int, keys: torch.Tensor) -> None:
        """``keys`` [n_probes, tokens, heads*d]: ``to_k(norm_cross(E_p))`` of every probe for layer ``layer`` (computed once per
        layer and trace by the processor; kept alive here until the engine closes)."""
        if keys.dim() != 3 or keys.shape[0] != self.n_probes or keys.shape[1] != self.tokens:
            raise ValueError(f'probe keys must be [{self.n_probes}, {self.tokens}, C], got {list(keys.shape)}')
        if layer in self._probe_k:
            self.flush()                                   # recorded taps still point at the old keys: launch them before those go
        self._probe_k[layer] = keys.contiguous()

    def _probe_desc_for(self, desc: 'nat.QKDesc') -> 'nat.QKDesc':
        """The descriptor of the probes' chains for a generation call described by ``desc``: the same Q, the same key layout
        with batch stride 0 (one probe key serves every kept batch entry)."""
        raw = bytes(desc)
        out = self._probe_desc.get(raw)
        if out is None:
            out = self._probe_desc[raw] = nat.QKDesc.from_buffer_copy(raw)
            out.k_stride_b = 0
        return out

    def _probe_key_ptr(self, layer: int, probe: int) -> int:
        keys = self._probe_k.get(layer)
        if keys is None:
            raise RuntimeError(f'daam_amd: layer {layer} was tapped before its probe keys were set')
        return keys.data_ptr() + probe * keys.stride(0) * keys.element_size()

    def _with_probes(self, layers: np.ndarray, qp: np.ndarray, kp: np.ndarray, dp: np.ndarray):
        """The recorded generation taps followed by every probe's taps of the same calls (same Q, the probe's K, slot
        ``probe_slot``): ``(n, [layers, q, k, desc])`` for ``daam_tap_qk_enqueue_many``."""
        uniq, inv = np.unique(dp, return_inverse=True)
        pdesc = np.array([ctypes.addressof(self._probe_desc_for(nat.QKDesc.from_address(int(a)))) for a in uniq], dtype=np.uint64)
        out_l, out_q, out_k, out_d = [layers], [qp], [kp], [dp]
        for p in range(self.n_probes):
            ptr = np.zeros(self.n_layers, dtype=np.uint64)
            for layer in np.unique(layers).tolist():
                ptr[layer] = self._probe_key_ptr(layer, p)
            out_l.append((layers + (1 + p) * self.n_layers).astype(np.int32))
            out_q.append(qp)
            out_k.append(ptr[layers])
            out_d.append(pdesc[inv])
        arrays = [np.ascontiguousarray(np.concatenate(a)) for a in (out_l, out_q, out_k, out_d)]
        return len(arrays[0]), arrays

    def tap_probes(self, layer: int, query: torch.Tensor, heads: int, scale: float, factor: int, round_logits: bool = True) -> None:
        """Immediate probe taps of one call (``daam_tap_qk`` per probe on ``query`` [B, hw, heads*d], the raw ``to_q`` output):
        the route of ``defer_steps=0``, ``DAAM_NO_ATTEND`` without deferral and the materialised processor.  The generation's own tap
        of the call comes first (it configures the layer); a probe never sees the generation's attention mask."""
        if self.defer_steps:
            # an immediate tap needs an empty queue.  On the materialised route of a deferred trace the generation's own tap_probs of
            # this call has just flushed it (daam_tap_probs takes no pending taps), so this adds no launch of its own
            self.flush()
        query = query if query.is_contiguous() else query.contiguous()
        b, hw, c = self._ensure_call_layer(layer, query, heads, factor)
        desc = _contiguous_qk_desc(query.dtype, b, heads, hw, self.tokens, c, scale, round_logits, k_stride_b=0)
        stream = self.stream
        for p in range(self.n_probes):
            nat.check(self.lib.daam_tap_qk(self.ctx, self.probe_slot(p, layer), query.data_ptr(), self._probe_key_ptr(layer, p),
                                           nat.byref(desc), stream))

    def probe_items(self, probe: int) -> Dict[Key, torch.Tensor]:
        """``{(factor, layer, head): probe ``probe``'s running sum [tokens, h, w]}`` -- views of the live buffers, with the lifetime
        rules of ``items``."""
        if not 0 <= probe < self.n_probes:
            raise IndexError(f'probe {probe} out of range: the trace has {self.n_probes} probe(s)')
        return dict(self._views(lambda layer: self.acc[self.probe_slot(probe, layer)]))

    def probe_heat_maps(self, probes: Sequence[int], n_prompts: int, n_rows: Sequence[int], factors: Optional[Sequence[int]] = None,
                        head_idx: Optional[int] = None, layer_idx: Optional[int] = None) -> torch.Tensor:
        """Global heat maps of the probes ``probes`` x ``n_prompts`` prompts from ONE ``daam_finalize_groups`` call (groups of 64 per
        call beyond that): returns ``[len(probes) * n_prompts, tokens, x, x]`` fp32, group ``i * n_prompts + j`` = probe ``probes[i]``
        seen by prompt ``j``, whose rows ``[0, n_rows[i])`` are its map."""
        table, _ = self._select(n_prompts, factors, head_idx, layer_idx, probes=probes, n_rows=n_rows)
        n_groups = len(probes) * n_prompts
        rows = [self._rows(n_rows[g // n_prompts]) for g in range(n_groups)]
        self.flush()
        i32 = ctypes.c_int32

        def call(start, n, out_ptr, plane):
            part = [g - start if start <= g < start + n else -1 for g in table]
            return self.lib.daam_finalize_groups(self.ctx, (i32 * len(part))(*part), n, (i32 * n)(*rows[start:start + n]), out_ptr, plane,
                                                 self.stream)
        return self._finalize_chunks(n_groups, call)

    def tap_probs(self, layer: int, probs: torch.Tensor, factor: int) -> None:
        """``probs`` [B*H, hw, tokens] as returned by ``get_attention_scores`` (trace.py:276).

        Arbitrary planes (not probabilities) may be fed this way, but the default finalize of 32 x 32 layers onto a 64 x 64 map runs on
        the matrix cores and has a value domain (include/daam_hip.h, finalize): the running sums must stay within ``|v| <= 2^15`` (no
        check; beyond it the map turns inf / NaN), and every map element carries an absolute error floor of 2^-23 on top of 2^-19 of its
        token row's maximum -- token rows summed far below 2^-10 lose their low bits.  ``DAAM_NO_PIPE_FINALIZE=1`` (bf16 / f32 sums) or
        ``DAAM_NO_MFMA_FINALIZE=1`` (fp16 sums), set before the trace starts, select the exact f32 kernels, which take any finite
        planes."""
        self._require_device(probs)
        self._ensure_ctx(probs.dtype)
        self.flush()
        probs = probs if probs.is_contiguous() else probs.contiguous()
        bh, hw, tokens = probs.shape
        self._ensure_layer(layer, bh - bh // 2, self._side(hw, factor), factor)
        nat.check(self.lib.daam_tap_probs(self.ctx, layer, probs.data_ptr(),
                                          _DTYPE_CODE[probs.dtype],
                                          bh, hw, tokens, self.stream))
        self._touch(layer)

    def add_map(self, factor: int, layer: int, head: int, heat_map: torch.Tensor) -> None:
        """``RawHeatMapCollection.update`` called by hand (heatmap.py:153-156): rare, done with a
        torch add on the layer's buffer.  The value domain of ``tap_probs`` applies to what the sums hold afterwards: 32 x 32 layers
        finalized onto a 64 x 64 map need ``|v| <= 2^15`` and carry an absolute error floor of 2^-23 per map element unless the exact
        route is selected (``DAAM_NO_PIPE_FINALIZE=1`` for bf16 / f32 sums, ``DAAM_NO_MFMA_FINALIZE=1`` for fp16 sums)."""
        if self.time_bins is not None:
            raise RuntimeError('daam_amd: update() is not supported on a trace with time_bins (which window would it add to?)')
        self._require_device(heat_map)
        self._ensure_ctx(heat_map.dtype)
        self.flush()
        t, h, w = heat_map.shape
        if layer not in self.layer_info:
            raise RuntimeError('daam_amd: update() on a layer that was never tapped is not supported')
        # clear() is lazy on the device side: the library zeroes the buffer now if it still owes that (on this
        # stream) and learns that the layer holds sums again (later taps add to them, the next reset clears them)
        nat.check(self.lib.daam_layer_touch(self.ctx, layer, self.stream))
        self.acc[layer][head] += heat_map.to(self.acc_dtype)
        self._touch(layer)

    # ---- views -----------------------------------------------------------------------------------
    def keys(self) -> List[Key]:
        out: List[Key] = []
        for layer in self.touched:
            factor, heads, _ = self.layer_info[layer]
            out += [(factor, layer, h) for h in range(heads)]
        return out

    def items(self) -> Iterator[Tuple[Key, torch.Tensor]]:
        """``((factor, layer, head), running sum [tokens, h, w])`` in first-update order.  The tensors are VIEWS of
        the live sum buffers (no 221 MB copy per iteration); they stay valid and unchanged after ``clear()`` / the
        end of the trace -- like the reference's tensors -- because an engine whose buffers were handed out starts its
        next generation on fresh buffers and does not park them for reuse.  Taps of the SAME generation that follow
        the iteration do show up in them."""
        if self.time_bins is not None:
            raise RuntimeError('daam_amd: a trace with time_bins keeps one sum per window: use raw_heat_maps(time_bin)')
        yield from self._views(lambda layer: self.acc[layer])

    def _views(self, buffer_of) -> Iterator[Tuple[Key, torch.Tensor]]:
        """The walk behind ``items`` / ``window_items`` / ``probe_items``: launch what is recorded, remember that views of the live
        buffers are out (``clear`` / ``close``), then every touched layer's ``buffer_of(layer)`` [heads, tokens, h, w] head by head."""
        self.flush()
        self._views_out = True
        for layer in list(self.touched):
            factor, heads, _ = self.layer_info[layer]
            buf = buffer_of(layer)
            for h in range(heads):
                yield (factor, layer, h), buf[h]

    def window_items(self, window: int) -> Dict[Key, torch.Tensor]:
        """``{(factor, layer, head): running sum of window ``window`` [tokens, h, w]}`` -- views of the live buffers, with the
        lifetime rules of ``items``.  A window the layer has not reached in this generation reads zero (``_zero_unreached_windows``)."""
        self._zero_unreached_windows()
        return dict(self._views(lambda layer: self.acc[layer][window]))

    def _zero_unreached_windows(self) -> None:
        """``clear()`` and the adoption of a parked context keep the sum buffers and ``daam_reset`` zeroes lazily: a slot is overwritten
        by its first tap, or cleared by the first finalize that covers it.  A window that a touched layer has not reached in this
        generation (a shorter generation, a layer tapped fewer times) gets neither before its view is handed out, and would show the
        previous generation's sums.  The engine knows which windows those are -- a layer tapped ``n`` times has reached the windows that
        start before step ``n`` -- and zeroes them here, once per layer and reset, on the current stream behind the launch of
        whatever was recorded.  The library still owes them its own zeroing; a later tap into one overwrites it (the slot is fresh)."""
        if self.time_bins is None:                         # no windows: items() hands out touched layers, which their first tap overwrote
            return
        layers = [layer for layer in self.touched if layer in self._stale]
        if not layers:
            return
        steps = self.tap_steps()                           # launches what is recorded first
        for layer in layers:
            reached = sum(1 for first in self.time_bins if first < steps[layer])
            if reached < self.n_bins:
                self.acc[layer][reached:].zero_()
            self._stale.discard(layer)

    def tap_steps(self) -> Dict[int, int]:
        """Taps each touched layer received since the last reset (``daam_tap_steps``; pending deferred taps are launched first)."""
        self.flush()
        if self.ctx is None:
            return {}
        n = ctypes.c_int()
        out = {}
        for layer in self.touched:
            nat.check(self.lib.daam_tap_steps(self.ctx, layer, ctypes.byref(n)))
            out[layer] = n.value
        return out

    def window_steps(self) -> List[int]:
        """Steps each time window received in the last generation (one entry without ``time_bins``)."""
        steps = list(self.tap_steps().values())
        if self.time_bins is None:
            return [max(steps, default=0)]
        return window_steps(self.time_bins, steps)

    def _binned(self, bins: Optional[Tuple[int, int]]) -> bool:
        """Does this selection take ``daam_finalize_bins``?  Only a trace of several windows: one window is the default layout
        (the library's un-binned calls, bit for bit)."""
        if self.n_bins > 1:
            return True
        if bins is not None and tuple(bins) != (0, 1):
            raise ValueError(f'time window range {bins} on a trace of one window')
        return False

    # ---- finalize ---------------------------------------------------------------------------------
    def _rows(self, n_rows) -> int:
        """The crop of trace.py:127 as the library takes it: 1 to ``tokens`` rows."""
        return max(1, min(int(n_rows), self.tokens))

    def _key_layout(self, slots: Sequence[int]) -> Tuple[int, List[int]]:
        """``(keys of the context, key offset of every slot of ``slots``)`` in the library's key order (configured slots by index,
        heads inside): ``daam_key_offset``."""
        total, off = ctypes.c_int(), ctypes.c_int()
        nat.check(self.lib.daam_key_offset(self.ctx, 0, None, ctypes.byref(total)))
        offsets = []
        for slot in slots:
            nat.check(self.lib.daam_key_offset(self.ctx, slot, ctypes.byref(off), None))
            offsets.append(off.value)
        return total.value, offsets

    def _select(self, n_sets: int, factors, head_idx, layer_idx, probes: Optional[Sequence[int]] = None, used=None,
                n_rows: Optional[Sequence[int]] = None, mask: bool = False):
        """What every finalize entry point decides before its library call.  Nothing tapped: LookupError.  ``n_rows`` (the grouped
        calls): one per prompt -- per probe with ``probes`` --, else ValueError.  Then the key -> group table of the selection:
        ``prompt_key_groups`` over the touched layers for ``n_sets`` prompts, or ``probe_key_groups`` over the slots of ``probes``
        (group = probe x prompt); cached per selection -- building it costs more host time than the finalize kernels take on the
        device -- as ``(table, its ctypes form, keys per group)``; the ctypes form is the int32 table, or with ``mask`` the byte mask
        ``table >= 0`` of ``daam_finalize``.  A group of ``used`` (default: every group) without a key: the recorded taps are still
        launched, then LookupError.  Returns ``(table, ctypes form)``; the caller flushes."""
        if self.ctx is None or not self.touched:
            raise LookupError('no heat maps')
        if n_rows is not None and len(n_rows) != (n_sets if probes is None else len(probes)):
            raise ValueError(f'{len(n_rows)} row counts for {n_sets} prompts' if probes is None else
                             f'{len(n_rows)} row counts for {len(probes)} probes')
        sel = (mask, None if probes is None else tuple(probes), n_sets, None if factors is None else tuple(sorted(set(factors))),
               head_idx, layer_idx, tuple(self.touched), len(self.layer_info))
        cached = self._mask_cache.get(sel)
        if cached is None:
            info = [self.layer_info[layer][:2] for layer in self.touched]
            if probes is None:
                total, offs = self._key_layout(self.touched)
                table = prompt_key_groups([(layer, off, *fh) for layer, off, fh in zip(self.touched, offs, info)], total, n_sets,
                                          factors, head_idx, layer_idx)
            else:
                where = [(i, layer, fh) for i in range(len(probes)) for layer, fh in zip(self.touched, info)]
                total, offs = self._key_layout([self.probe_slot(probes[i], layer) for i, layer, _ in where])
                table = probe_key_groups([(i, layer, off, *fh) for (i, layer, fh), off in zip(where, offs)], total, len(probes),
                                         n_sets, factors, head_idx, layer_idx)
            counts = [table.count(g) for g in range(n_sets * (1 if probes is None else len(probes)))]
            form = (ctypes.c_uint8 * total)(*[g >= 0 for g in table]) if mask else (ctypes.c_int32 * total)(*table)
            if len(self._mask_cache) > 64:
                self._mask_cache.clear()
            cached = self._mask_cache[sel] = (table, form, counts)
        table, form, counts = cached
        if any(counts[g] == 0 for g in (range(len(counts)) if used is None else used)):
            self.flush()
            raise LookupError('no heat maps')
        return table, form

    def _finalize_chunks(self, n_groups: int, call) -> torch.Tensor:
        """``[n_groups, tokens, out_h, out_w]`` fp32 from a grouped finalize that takes at most 64 groups per call:
        ``call(first group, groups, output address of the first, group stride)`` returns the library's status."""
        plane = self.tokens * self.out_h * self.out_w
        out = torch.empty(n_groups, self.tokens, self.out_h, self.out_w, dtype=torch.float32, device=self.device)
        for start in range(0, n_groups, 64):
            nat.check(call(start, min(64, n_groups - start), out.data_ptr() + start * plane * 4, plane))
        return out

    def global_heat_map(self, factors: Optional[Sequence[int]] = None, head_idx: Optional[int] = None,
                        layer_idx: Optional[int] = None, n_rows: Optional[int] = None,
                        bins: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """trace.py:103-126: returns ``[n_rows, x, x]`` fp32 on the device.  ``n_rows`` (default: every token row) is the
        crop of trace.py:127 applied BEFORE the work: the planes of the token rows nobody reads are neither fetched nor
        written (``daam_finalize``'s ``n_rows``, ABI v6).  ``bins`` = ``(first, end)`` window range of a trace with ``time_bins``
        (default: the whole generation)."""
        binned = self._binned(bins)
        rows = self.tokens if n_rows is None else self._rows(n_rows)
        if binned:
            b0, b1 = bins if bins is not None else (0, self.n_bins)
            return self.time_heat_maps([(b0, b1, 0)], 1, [rows], factors, head_idx, layer_idx)[0, :rows]
        factors = None if factors is None else set(factors)         # a factors argument that is no iterable fails first, as ever
        # the key mask in the library's key order: the one-prompt table, ``>= 0``
        _, mask = self._select(1, factors, head_idx, layer_idx, mask=True)
        out = torch.empty(rows, self.out_h, self.out_w, dtype=torch.float32, device=self.device)
        if self.rect:
            # no announcement on a non-square map (daam_finalize_prepare is DAAM_E_UNSUPPORTED there): the finalize clears its output
            self.flush()
            nat.check(self.lib.daam_finalize(self.ctx, mask, rows, out.data_ptr(), self.stream))
            return out
        # the output is announced BEFORE the deferred taps go out: the launch's table-upload kernel clears it and the key tables
        # stay on the device between generations, so the finalize call below is its class kernel(s) only (daam_finalize_prepare)
        optr = out.data_ptr()

        def announce(stream):
            nat.check(self.lib.daam_finalize_prepare(self.ctx, mask, rows, optr, stream))
        if not self.flush(_before_launch=announce):
            announce(self.stream)
        nat.check(self.lib.daam_finalize(self.ctx, mask, rows, optr, self.stream))
        return out

    def key_groups(self, n_groups: int, factors: Optional[Sequence[int]] = None, head_idx: Optional[int] = None,
                   layer_idx: Optional[int] = None) -> List[int]:
        """The prompt of every key in the library's key order (-1: not selected), for ``n_groups`` prompts traced in one batch
        under classifier-free guidance: a layer's kept keys are ``[cond x N*k]`` batch items of H heads each, so prompt ``p``
        owns the block ``[p * kept/N, (p+1) * kept/N)``.  ``head_idx`` counts inside a prompt's block (the reference's
        ``head_idx`` on a single prompt), ``factors`` / ``layer_idx`` filter as in ``global_heat_map``."""
        total, offs = self._key_layout(self.touched)
        layout = [(layer, off, *self.layer_info[layer][:2]) for layer, off in zip(self.touched, offs)]
        return prompt_key_groups(layout, total, n_groups, factors, head_idx, layer_idx)

    def global_heat_maps(self, n_groups: int, n_rows: Sequence[int], factors: Optional[Sequence[int]] = None,
                         head_idx: Optional[int] = None, layer_idx: Optional[int] = None,
                         bins: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """One global heat map per prompt of a batched generation, in ONE ``daam_finalize_groups`` call: returns
        ``[n_groups, tokens, x, x]`` fp32 whose rows ``[0, n_rows[p])`` of prompt ``p`` are its map (the others are not written).
        ``bins``: window range, as in ``global_heat_map``."""
        if self._binned(bins):
            if len(n_rows) != n_groups:
                raise ValueError(f'{len(n_rows)} row counts for {n_groups} prompts')
            b0, b1 = bins if bins is not None else (0, self.n_bins)
            return self.time_heat_maps([(b0, b1, p) for p in range(n_groups)], n_groups, n_rows, factors, head_idx, layer_idx)
        _, table = self._select(n_groups, factors, head_idx, layer_idx, n_rows=n_rows)
        rows = [self._rows(r) for r in n_rows]
        self.flush()
        out = torch.empty(n_groups, self.tokens, self.out_h, self.out_w, dtype=torch.float32, device=self.device)
        nat.check(self.lib.daam_finalize_groups(self.ctx, table, n_groups, (ctypes.c_int32 * n_groups)(*rows), out.data_ptr(),
                                                self.tokens * self.out_h * self.out_w, self.stream))
        return out

    def time_heat_maps(self, groups: Sequence[Tuple[int, int, int]], n_prompts: int, n_rows: Sequence[int],
                       factors: Optional[Sequence[int]] = None, head_idx: Optional[int] = None,
                       layer_idx: Optional[int] = None) -> torch.Tensor:
        """Global heat maps of ``(first window, end window, prompt)`` groups (``daam_finalize_bins``, at most 64 groups per call):
        returns ``[len(groups), tokens, x, x]`` fp32 whose rows ``[0, n_rows[prompt])`` of each group are its map.  ``n_prompts``
        prompts share the key table (``key_groups``); the filters are per prompt."""
        _, table = self._select(n_prompts, factors, head_idx, layer_idx, used=(p for _, _, p in groups), n_rows=n_rows)
        rows = [self._rows(r) for r in n_rows]
        self.flush()

        def call(start, n, out_ptr, plane):
            part = groups[start:start + n]
            i32 = ctypes.c_int32 * n
            return self.lib.daam_finalize_bins(self.ctx, table, n, i32(*[p for _, _, p in part]), i32(*[b for b, _, _ in part]),
                                               i32(*[e for _, e, _ in part]), i32(*[rows[p] for _, _, p in part]), out_ptr, plane,
                                               self.stream)
        return self._finalize_chunks(len(groups), call)

    def key_scores(self, footprint: Optional[torch.Tensor] = None, n_rows: Optional[int] = None,
                   factors: Optional[Sequence[int]] = None, head_idx: Optional[int] = None, layer_idx: Optional[int] = None,
                   n_prompts: int = 1, prompt: int = 0, bins: Optional[Tuple[int, int]] = None):
        """Head analysis (``daam_key_scores`` of ``libdaam_analysis.so``): per selected key the finalize's arithmetic -- bicubic to the
        map's size, clamp at 0 -- ending in a dot product with each ``footprint`` [M, out_h, out_w] (fp32, what ``region_scores`` /
        ``RegionAttribution.footprint`` hold; ``None``: the total clamped mass, one column) instead of the sum over keys.  Returns
        ``(keys, scores)``: ``keys`` the ``(factor, layer, head)`` of prompt ``prompt``'s selection in the library's key order
        (``head`` counts inside the prompt's block, like ``head_idx``), ``scores`` fp32 ``[len(keys), max(M, 1), rows]`` on the device.
        One launch per 32 footprints reads the running sums once and writes no map; the filters, ``n_rows`` and ``bins`` mean what they
        mean in ``global_heat_maps``.  The mean of ``scores`` over the keys is, by linearity, ``region_dots`` of the global map."""
        rows, planes = self._key_selection(n_rows, factors, head_idx, layer_idx, n_prompts, prompt, bins)
        if footprint is not None:
            if footprint.dtype != torch.float32 or footprint.dim() != 3 or tuple(footprint.shape[1:]) != (self.out_h, self.out_w) \
                    or footprint.shape[0] < 1:
                raise ValueError(f'footprint must be fp32 [M, {self.out_h}, {self.out_w}], got {tuple(footprint.shape)} {footprint.dtype}')
            if footprint.device != self.device:
                raise RuntimeError('daam_amd: the footprint is not on the engine\'s device')
            footprint = footprint.contiguous()
        keys, desc = self._key_planes(*planes)
        lib = nat.load_analysis()
        parts = []
        chunks = [None] if footprint is None else [footprint[at:at + MAX_REGION_MASKS] for at in range(0, footprint.shape[0], MAX_REGION_MASKS)]
        with torch.cuda.device(self.device):
            for chunk in chunks:
                m = 0 if chunk is None else chunk.shape[0]
                scores = torch.empty(len(keys), max(m, 1), rows, dtype=torch.float32, device=self.device)
                nat.check_analysis(lib.daam_key_scores(desc.data_ptr(), len(keys), _DTYPE_CODE[self.acc_dtype], rows, self.out_h, self.out_w,
                                                       None if chunk is None else chunk.data_ptr(), m, scores.data_ptr(), self.stream))
                parts.append(scores)
        return keys, parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)

    def token_gram(self, n_rows: Optional[int] = None, factors: Optional[Sequence[int]] = None, head_idx: Optional[int] = None,
                   layer_idx: Optional[int] = None, n_prompts: int = 1, prompt: int = 0, bins: Optional[Tuple[int, int]] = None):
        """Token co-attention (``daam_token_gram`` of ``libdaam_analysis.so``): per selected key the Gram matrix of its token planes,
        ``gram[k][i][j] = sum_p plane_i[p] * plane_j[p]``, at the key's own resolution from the raw running sums (no bicubic, no
        clamp), from one pass over the sums that ends on the matrix cores.  ``key_scores`` without footprints: the same selection,
        key order, ``n_rows`` crop, ``bins`` and ``LookupError``.  Returns ``(keys, gram)`` with ``gram`` fp32
        ``[len(keys), rows, rows]`` on the device.  The scratch of the keys' partial matrices is the engine's, grown on demand."""
        rows, planes = self._key_selection(n_rows, factors, head_idx, layer_idx, n_prompts, prompt, bins)
        keys, desc = self._key_planes(*planes)
        lib = nat.load_analysis()
        # sized for the largest touched layer, selected or not (60 layers to look at, not 1100 keys; more scratch changes no bit)
        sides = {self.layer_info[layer][2] for layer in self.touched}
        max_hw = max(s[0] * s[1] if isinstance(s, tuple) else s * s for s in sides)
        need = lib.daam_token_gram_scratch_bytes(len(keys), rows, max_hw)
        if need == 0:
            raise ValueError(f'daam_token_gram takes 1..96 token rows and up to 2^20 keys, got {rows} rows of {len(keys)} keys')
        with torch.cuda.device(self.device):
            if self._gram_scratch is None or self._gram_scratch.numel() < need:
                self._gram_scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
            gram = torch.empty(len(keys), rows, rows, dtype=torch.float32, device=self.device)
            nat.check_analysis(lib.daam_token_gram(desc.data_ptr(), len(keys), _DTYPE_CODE[self.acc_dtype], rows, gram.data_ptr(),
                                                   self._gram_scratch.data_ptr(), self._gram_scratch.numel(), self.stream))
        return keys, gram

    def key_blend(self, weights: torch.Tensor, n_rows: Optional[int] = None, factors: Optional[Sequence[int]] = None,
                  head_idx: Optional[int] = None, layer_idx: Optional[int] = None, n_prompts: int = 1, prompt: int = 0,
                  bins: Optional[Tuple[int, int]] = None):
        """Heat maps of weighted key sets (``daam_key_blend`` of ``libdaam_analysis.so``): the finalize's arithmetic -- bicubic to the
        map's size, clamp at 0 -- with ``weights[g][k]`` in front of the sum over keys, ``maps[g] = sum_k weights[g][k] * K_k``.
        ``weights`` is fp32 ``[G, len(keys)]`` in the key order of ``key_scores`` for the same selection (a host tensor is moved to
        the device); a zero weight is no contribution and a key every set weighs 0 is not read.  Returns ``(keys, maps)`` with
        ``maps`` fp32 ``[G, rows, out_h, out_w]`` on the device; one call per 8 sets reads the running sums once.  The selection,
        key order, ``n_rows`` crop, ``bins`` and ``LookupError`` are ``key_scores``'.  The scratch is the engine's, grown on demand."""
        rows, planes = self._key_selection(n_rows, factors, head_idx, layer_idx, n_prompts, prompt, bins)
        keys, desc = self._key_planes(*planes)
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or weights.dim() != 2 \
                or weights.shape[1] != len(keys) or weights.shape[0] < 1:
            got = f'{tuple(weights.shape)} {weights.dtype}' if isinstance(weights, torch.Tensor) else type(weights).__name__
            raise ValueError(f'weights must be fp32 [G, {len(keys)}] (one column per selected key), got {got}')
        weights = weights.to(self.device).contiguous()
        lib = nat.load_analysis()
        n_sets, cells = weights.shape[0], self.out_h * self.out_w
        need = lib.daam_key_blend_scratch_bytes(len(keys), min(n_sets, MAX_BLEND_SETS), rows, self.out_h, self.out_w)
        if need == 0:
            raise ValueError(f'daam_key_blend takes up to 2^20 keys and maps of up to 128 x 128, got {len(keys)} keys, {rows} rows of '
                             f'{self.out_h} x {self.out_w}')
        with torch.cuda.device(self.device):
            if self._blend_scratch is None or self._blend_scratch.numel() < need:
                self._blend_scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
            maps = torch.empty(n_sets, rows, self.out_h, self.out_w, dtype=torch.float32, device=self.device)
            for at in range(0, n_sets, MAX_BLEND_SETS):
                n = min(MAX_BLEND_SETS, n_sets - at)
                nat.check_analysis(lib.daam_key_blend(desc.data_ptr(), len(keys), _DTYPE_CODE[self.acc_dtype], rows, self.out_h, self.out_w,
                                                      weights[at:at + n].data_ptr(), n, maps[at:at + n].data_ptr(), rows * cells,
                                                      self._blend_scratch.data_ptr(), self._blend_scratch.numel(), self.stream))
        return keys, maps

    def _key_selection(self, n_rows, factors, head_idx, layer_idx, n_prompts, prompt, bins):
        """What ``key_scores`` and ``token_gram`` decide before they build descriptors: ``(rows, planes)`` -- the ``n_rows`` crop and
        the arguments of ``_key_planes`` for prompt ``prompt``'s selection over the window range ``bins`` (the caller makes that call,
        after the checks of its own arguments).  ValueError for a prompt out of range, then ``_select``'s LookupError; the recorded
        taps are launched either way."""
        binned = self._binned(bins)
        rows = self.tokens if n_rows is None else self._rows(n_rows)
        n_prompts, prompt = int(n_prompts), int(prompt)
        if not 0 <= prompt < n_prompts:
            raise ValueError(f'prompt {prompt} of {n_prompts}')
        factors = None if factors is None else set(factors)
        table, _ = self._select(n_prompts, factors, head_idx, layer_idx, used=(prompt,))
        self.flush()
        b0, b1 = (bins if bins is not None else (0, self.n_bins)) if binned else (0, 1)
        return rows, (table, n_prompts, prompt, factors, head_idx, layer_idx, b0, b1, binned)

    def _key_planes(self, table, n_prompts, prompt, factors, head_idx, layer_idx, b0, b1, binned):
        """``(keys, DaamKeyPlanes[len(keys)] as a uint8 device tensor)`` of prompt ``prompt``'s keys in ``table``, in the library's key
        order.  Base pointers are those of the views ``items()`` / ``window_items(b0)`` yield (the sums are addressed nowhere else);
        a window range is ``n_win = b1 - b0`` and the distance of a key's views in two windows.  Cached per selection, window range and
        buffer addresses: 1100 ``data_ptr()`` calls cost more host time than the kernel takes."""
        sel = (n_prompts, prompt, None if factors is None else tuple(sorted(factors)), head_idx, layer_idx, b0, b1, tuple(self.touched),
               tuple(self.acc[layer].data_ptr() for layer in self.touched))
        cached = self._ks_cache.get(sel)
        if cached is not None:
            if binned:
                self._zero_unreached_windows()
            return cached
        views_out = self._views_out                        # the views stay in here: the buffers may still be parked for reuse
        windows = self.time_bins is not None               # one window is still laid out [1, heads, ...]
        first = self.window_items(b0) if windows else dict(self.items())
        second = self.window_items(b0 + 1) if b1 - b0 > 1 else None
        self._views_out = views_out
        _, offs = self._key_layout(self.touched)
        picked = []
        for layer, off in zip(self.touched, offs):
            factor, heads, _ = self.layer_info[layer]
            block = heads // n_prompts
            for h in range(heads):
                if table[off + h] == prompt:
                    view = first[(factor, layer, h)]
                    if not view.is_contiguous():
                        raise RuntimeError('daam_amd: a running sum is not contiguous')
                    stride = 0 if second is None else (second[(factor, layer, h)].data_ptr() - view.data_ptr()) // view.element_size()
                    picked.append((off + h, (factor, layer, h - prompt * block), view, stride))
        picked.sort(key=lambda e: e[0])
        arr = (nat.KeyPlanes * len(picked))()
        for i, (_, _, view, stride) in enumerate(picked):
            arr[i] = nat.KeyPlanes(base=view.data_ptr(), win_stride=stride, h=view.shape[-2], w=view.shape[-1], n_win=b1 - b0, pad=0)
        desc = _descriptors_on(self.device, arr)
        if len(self._ks_cache) > 16:
            self._ks_cache.clear()
        cached = self._ks_cache[sel] = ([key for _, key, _, _ in picked], desc)
        return cached

    def normalize_(self, maps: torch.Tensor) -> torch.Tensor:
        """trace.py:129-130, in place on ``maps`` [n_rows, x, x] -- or [n_rows, out_h, out_w] -- (contiguous fp32)."""
        h, w = maps.shape[-2:]
        if h == w:
            nat.check(self.lib.daam_epilogue_normalize(maps.data_ptr(), maps.shape[0], w, self.stream))
        else:
            nat.check(self.lib.daam_epilogue_normalize_rect(maps.data_ptr(), maps.shape[0], h, w, self.stream))
        return maps


def prompt_key_groups(layout: Sequence[Tuple[int, int, int, int]], total: int, n_groups: int,
                      factors: Optional[Sequence[int]] = None, head_idx: Optional[int] = None,
                      layer_idx: Optional[int] = None) -> List[int]:
    """``daam_finalize_groups``' key -> prompt table.  ``layout`` = ``(layer, key offset, factor, kept heads)`` of every tapped
    layer; a layer's kept keys are the conditional half ``[cond x N*k]`` of H heads each, so prompt ``p`` owns
    ``[p * kept/N, (p+1) * kept/N)``; ``head_idx`` counts inside that block."""
    fset = {0, 1, 2, 4, 8, 16, 32, 64} if factors is None else set(factors)
    groups = [-1] * total
    for layer, off, factor, heads in layout:
        if factor not in fset or (layer_idx is not None and layer_idx != layer):
            continue
        if heads % n_groups:
            raise ValueError(f'layer {layer} keeps {heads} batch*heads entries, not divisible by {n_groups} prompts')
        block = heads // n_groups
        for p in range(n_groups):
            for h in range(block):
                if head_idx is None or head_idx == h:
                    groups[off + p * block + h] = p
    return groups


def _launch_word(src: torch.Tensor, idxs: Sequence[int], word: torch.Tensor, out: Optional[torch.Tensor], absolute: bool,
                 threshold: float) -> None:
    """``daam_word_heat_map`` on square planes ``src`` [rows, s, s], ``daam_word_heat_map_rect`` on [rows, h, w]: the one place that
    chooses between them.  ``word`` takes the mean of the planes ``idxs``, ``out`` (or None) its resize."""
    lib = nat.load()
    h, w = src.shape[-2:]
    fn, size = (lib.daam_word_heat_map, (h,)) if h == w else (lib.daam_word_heat_map_rect, (h, w))
    ws = torch.empty(2, dtype=torch.float32, device=src.device)
    out_ptr, out_h, out_w = (None, 0, 0) if out is None else (out.data_ptr(), out.shape[0], out.shape[1])
    nat.check(fn(src.data_ptr(), *size, (ctypes.c_int32 * len(idxs))(*[int(i) for i in idxs]), len(idxs), word.data_ptr(), out_ptr,
                 out_h, out_w, 1 if absolute else 0, threshold, ws.data_ptr(), torch.cuda.current_stream(src.device).cuda_stream))


def word_heat_map(maps: torch.Tensor, idxs: Sequence[int]) -> torch.Tensor:
    """heatmap.py:121-123: mean of the planes ``idxs`` of ``maps`` [rows, s, s] -> [s, s] (or [rows, h, w] -> [h, w])."""
    _check_maps(maps)
    for i in idxs:
        if not 0 <= int(i) < maps.shape[0]:
            raise IndexError(f'index {i} is out of bounds for dimension 0 with size {maps.shape[0]}')
    word = torch.empty(maps.shape[-2], maps.shape[-1], dtype=torch.float32, device=maps.device)
    _launch_word(maps, idxs, word, None, True, 0.0)
    return word


def expand_word_map(word: torch.Tensor, out_h: int, out_w: int, absolute: bool = False,
                    threshold: Optional[float] = None) -> torch.Tensor:
    """heatmap.py:77-93 up to (not including) the ``.cpu()``: bicubic to ``out_h x out_w``,
    min-max normalise unless ``absolute``, optional threshold."""
    if word.device.type != 'cuda' or word.dtype != torch.float32 or word.dim() != 2:
        raise RuntimeError('daam_amd: expand_as needs an fp32 [h, w] word map on the HIP device')
    word = word.contiguous()
    out = torch.empty(out_h, out_w, dtype=torch.float32, device=word.device)
    _launch_word(word, [0], torch.empty_like(word), out, absolute, float(threshold) if threshold else 0.0)
    return out


MAX_MASK_WORDS, MAX_MASK_INDICES = 32, 255        # limits of one daam_word_masks call (include/daam_hip.h)


def word_masks(maps: torch.Tensor, idx_lists: Sequence[Sequence[int]], out_h: int, out_w: int, absolute: bool = False,
               threshold: float = 0.4, labels: bool = True):
    """``daam_word_masks``: for up to 32 words (``idx_lists[j]`` = the planes of ``maps`` [rows, h, w] word ``j`` is the mean of) the
    mean planes ``word_maps`` [n, h, w] fp32, the masks ``expand_as(threshold=) > threshold`` as uint8 [n, out_h, out_w] and, with
    ``labels``, the uint8 [out_h, out_w] map of the word with the largest value at each pixel (lowest index on a tie, 255 where no
    word exceeds the threshold) -- three launches, all results on the device.  Returns ``(word_maps, masks, labels or None)``."""
    _check_maps(maps)
    idx_lists = [[int(i) for i in idxs] for idxs in idx_lists]
    n = len(idx_lists)
    if not 1 <= n <= MAX_MASK_WORDS:
        raise ValueError(f'word_masks takes 1..{MAX_MASK_WORDS} words per call, got {n}')
    flat, begin = [], [0]
    for idxs in idx_lists:
        if not idxs:
            raise ValueError('word_masks: a word with no token indices')
        for i in idxs:
            if not 0 <= i < maps.shape[0]:
                raise IndexError(f'index {i} is out of bounds for dimension 0 with size {maps.shape[0]}')
        flat += idxs
        begin.append(len(flat))
    if len(flat) > MAX_MASK_INDICES:
        raise ValueError(f'word_masks takes at most {MAX_MASK_INDICES} token indices per call, got {len(flat)}')
    rows, h, w = maps.shape
    out_h, out_w = int(out_h), int(out_w)
    word_maps = torch.empty(n, h, w, dtype=torch.float32, device=maps.device)
    masks = torch.empty(n, out_h, out_w, dtype=torch.uint8, device=maps.device)
    label_map = torch.empty(out_h, out_w, dtype=torch.uint8, device=maps.device) if labels else None
    ws = torch.empty(2 * n, dtype=torch.float32, device=maps.device)
    nat.check(nat.load().daam_word_masks(
        maps.data_ptr(), rows, h, w, (ctypes.c_int32 * len(flat))(*flat), (ctypes.c_int32 * len(begin))(*begin), n, word_maps.data_ptr(),
        out_h, out_w, 1 if absolute else 0, float(threshold), masks.data_ptr(), label_map.data_ptr() if labels else None, ws.data_ptr(),
        torch.cuda.current_stream(maps.device).cuda_stream))
    return word_maps, masks, label_map


def word_maps(maps: torch.Tensor, idx_lists: Sequence[Sequence[int]]) -> torch.Tensor:
    """The mean planes alone, fp32 [len(idx_lists), h, w]: ``daam_word_masks`` without masks or labels (one launch per 32 words or
    255 indices), so the planes are the ones ``word_masks`` returns, bit for bit."""
    _check_maps(maps)
    idx_lists = [[int(i) for i in idxs] for idxs in idx_lists]
    rows, h, w = maps.shape
    out = torch.empty(len(idx_lists), h, w, dtype=torch.float32, device=maps.device)
    ws = torch.empty(2 * MAX_MASK_WORDS, dtype=torch.float32, device=maps.device)
    first = 0
    while first < len(idx_lists):
        flat, begin = [], [0]
        for idxs in idx_lists[first:first + MAX_MASK_WORDS]:
            if not idxs:
                raise ValueError('word_maps: a word with no token indices')
            for i in idxs:
                if not 0 <= i < rows:
                    raise IndexError(f'index {i} is out of bounds for dimension 0 with size {rows}')
            if len(idxs) > MAX_MASK_INDICES:
                raise ValueError(f'word_maps: a word of {len(idxs)} token indices, at most {MAX_MASK_INDICES}')
            if len(flat) + len(idxs) > MAX_MASK_INDICES:
                break
            flat += idxs
            begin.append(len(flat))
        n = len(begin) - 1
        nat.check(nat.load().daam_word_masks(
            maps.data_ptr(), rows, h, w, (ctypes.c_int32 * len(flat))(*flat), (ctypes.c_int32 * len(begin))(*begin), n,
            out[first:].data_ptr(), 1, 1, 1, 0.0, None, None, ws.data_ptr(), torch.cuda.current_stream(maps.device).cuda_stream))
        first += n
    return out


MAX_SWEEP_WORDS, MAX_SWEEP_TRUTH, MAX_SWEEP_THRESHOLDS = 32, 32, 64        # limits of one daam_threshold_sweep call (include/daam_eval.h)


def _launch_threshold_sweep(planes: torch.Tensor, out_h: int, out_w: int, absolute: bool, thresholds: Sequence[float],
                            truth: Optional[torch.Tensor]):
    """One ``daam_threshold_sweep`` call: ``planes`` [W <= 32, h, w] fp32, ``thresholds`` <= 64 ascending floats, ``truth``
    [G <= 32, out_h, out_w] uint8 or None -> int32 ``(pred_area [W, T], inter [W, G, T] or None, truth_area [G] or None)``.  The
    counts are below 2^31."""
    lib = nat.load_eval()
    n, h, w = planes.shape
    g, t = 0 if truth is None else truth.shape[0], len(thresholds)
    dev = planes.device
    pred = torch.empty(n, t, dtype=torch.int32, device=dev)
    inter = torch.empty(n, g, t, dtype=torch.int32, device=dev) if g else None
    area = torch.empty(g, dtype=torch.int32, device=dev) if g else None
    need = lib.daam_threshold_sweep_workspace(n, g, t, out_h, out_w)
    if not need:
        raise ValueError(f'threshold sweep of {n} words, {g} truth masks, {t} thresholds at {out_h} x {out_w}: out of range')
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nat.check_eval(lib.daam_threshold_sweep(
            planes.data_ptr(), n, h, w, out_h, out_w, 1 if absolute else 0, (ctypes.c_float * t)(*thresholds), t,
            truth.data_ptr() if g else None, g, pred.data_ptr(), inter.data_ptr() if g else None, area.data_ptr() if g else None,
            ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream))
    return pred, inter, area


def threshold_sweep(word_maps: torch.Tensor, out_h: int, out_w: int, thresholds, truth: Optional[torch.Tensor] = None,
                    absolute: bool = False):
    """``daam_threshold_sweep``: what ``word_masks(threshold=t)`` followed by ``mask_overlap_matrix`` counts, for every ``t`` of
    ``thresholds`` at once.  ``word_maps`` [W, h, w] fp32 are the un-expanded mean planes (``word_maps()``, or the first result of
    ``word_masks``), ``truth`` [G, out_h, out_w] (or [out_h, out_w]) uint8 / bool masks (a byte != 0 is set; other dtypes through
    ``!= 0``; CPU masks are moved to the device) or None.  Returns int32 device tensors ``(area_pred [W, T], intersection
    [W, G, T] or None, area_truth [G] or None)``, the thresholds in the caller's order: they go to the device sorted and without
    duplicates (as f32), and more than 32 words, 32 truth masks or 64 distinct thresholds run in blocks that are stitched on the
    device.  Two passes at image resolution per block whatever the number of thresholds; no plane of out_h x out_w is written."""
    from .evaluate import _as_masks
    _check_maps(word_maps)
    out_h, out_w = int(out_h), int(out_w)
    thr = np.asarray(thresholds.detach().cpu().numpy() if isinstance(thresholds, torch.Tensor) else thresholds, dtype=np.float32).reshape(-1)
    if thr.size == 0 or not np.isfinite(thr).all():
        raise ValueError('threshold_sweep needs at least one threshold, all of them finite')
    if word_maps.shape[0] < 1:
        raise ValueError('threshold_sweep needs at least one word map')
    uniq, inverse = np.unique(thr, return_inverse=True)
    if truth is not None:
        truth = _as_masks(truth, 'truth', word_maps.device)
        if truth.device != word_maps.device:
            raise RuntimeError('daam_amd: word maps and truth masks are on different devices')
        if tuple(truth.shape[1:]) != (out_h, out_w):
            raise ValueError(f'truth masks of {tuple(truth.shape[1:])} for an output of {(out_h, out_w)}: threshold_sweep does not resize them')
    truth_blocks = [None] if truth is None else [truth[g:g + MAX_SWEEP_TRUTH] for g in range(0, truth.shape[0], MAX_SWEEP_TRUTH)]
    thr_blocks = [[float(t) for t in uniq[k:k + MAX_SWEEP_THRESHOLDS]] for k in range(0, uniq.size, MAX_SWEEP_THRESHOLDS)]
    pred_rows, inter_rows, areas = [], [], []
    for i in range(0, word_maps.shape[0], MAX_SWEEP_WORDS):
        pred_cols, inter_cols = [], []
        for ts in thr_blocks:
            parts = [_launch_threshold_sweep(word_maps[i:i + MAX_SWEEP_WORDS], out_h, out_w, absolute, ts, tb) for tb in truth_blocks]
            pred_cols.append(parts[0][0])
            if truth is not None:
                inter_cols.append(torch.cat([p[1] for p in parts], dim=1))
                if not areas:
                    areas = [p[2] for p in parts]
        pred_rows.append(torch.cat(pred_cols, dim=1))
        if truth is not None:
            inter_rows.append(torch.cat(inter_cols, dim=2))
    order = torch.as_tensor(np.ascontiguousarray(inverse.reshape(-1)), dtype=torch.long).to(word_maps.device)
    pred = torch.cat(pred_rows).index_select(1, order)
    if truth is None:
        return pred, None, None
    return pred, torch.cat(inter_rows).index_select(2, order), torch.cat(areas)


MAX_LOCATE_WORDS, MAX_LOCATE_TRUTH, MAX_LOCATE_THRESHOLDS = 32, 32, 64     # limits of one daam_localize call (include/daam_locate.h)


def _launch_localize(planes: Optional[torch.Tensor], out_h: int, out_w: int, absolute: bool, thresholds: Sequence[float],
                     truth: Optional[torch.Tensor]):
    """One ``daam_localize`` call: ``planes`` [W <= 32, h, w] fp32 or None, ``thresholds`` <= 64 floats in any order, ``truth``
    [G <= 32, out_h, out_w] uint8 or None -> ``(boxes int32 [W, T, 4], peaks int32 [W, 2], peak_values f32 [W, 3], truth_boxes int32
    [G, 4] or None, hits uint8 [W, G] or None)``; the first three are None without planes."""
    lib = nat.load_locate()
    n, h, w = (0, 1, 1) if planes is None else planes.shape
    g, t = 0 if truth is None else truth.shape[0], len(thresholds)
    dev = truth.device if planes is None else planes.device
    boxes = torch.empty(n, t, 4, dtype=torch.int32, device=dev) if n else None
    peaks = torch.empty(n, 2, dtype=torch.int32, device=dev) if n else None
    values = torch.empty(n, 3, dtype=torch.float32, device=dev) if n else None
    truth_boxes = torch.empty(g, 4, dtype=torch.int32, device=dev) if g else None
    hits = torch.empty(n, g, dtype=torch.uint8, device=dev) if n and g else None
    need = lib.daam_localize_workspace(n, g, t, out_h, out_w)
    if not need:
        raise ValueError(f'localize of {n} words, {g} truth masks, {t} thresholds at {out_h} x {out_w}: out of range')
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        nat.check_locate(lib.daam_localize(
            planes.data_ptr() if n else None, n, h, w, out_h, out_w, 1 if absolute else 0, (ctypes.c_float * max(t, 1))(*thresholds), t,
            truth.data_ptr() if g else None, g, boxes.data_ptr() if n and t else None, peaks.data_ptr() if n else None,
            values.data_ptr() if n else None, truth_boxes.data_ptr() if g else None, hits.data_ptr() if n and g else None,
            ws.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream))
    return boxes, peaks, values, truth_boxes, hits


def localize(word_maps: torch.Tensor, out_h: int, out_w: int, thresholds=(), truth: Optional[torch.Tensor] = None,
             absolute: bool = False):
    """``daam_localize``: per word and threshold the bounding box of the mask ``word_masks(threshold=t)`` gives, every word's peak
    (the arg-max of its expanded map) and whether it lies inside each truth mask, from one pass at image resolution whatever the
    number of thresholds.  ``word_maps`` [W, h, w] fp32 are the un-expanded mean planes (``word_maps()``), ``truth`` [G, out_h,
    out_w] (or [out_h, out_w]) uint8 / bool masks (a byte != 0 is set; other dtypes through ``!= 0``; CPU masks are moved to the
    device) or None.  Returns device tensors ``(boxes int32 [W, T, 4] -- x0 y0 x1 y1 inclusive, (out_w, out_h, -1, -1) when empty --,
    peaks int32 [W, 2] -- x, y --, peak_values f32 [W, 3] -- the raw expanded value at the peak, the minimum, the maximum --,
    truth_boxes int32 [G, 4] or None, hits bool [W, G] or None)``.  The thresholds are taken as they come (any order, duplicates
    allowed); more than 32 words, 32 truth masks or 64 thresholds run in blocks that are stitched on the device."""
    from .evaluate import _as_masks
    _check_maps(word_maps)
    out_h, out_w = int(out_h), int(out_w)
    thr = np.asarray(thresholds.detach().cpu().numpy() if isinstance(thresholds, torch.Tensor) else thresholds, dtype=np.float32).reshape(-1)
    if not np.isfinite(thr).all():
        raise ValueError('localize needs finite thresholds')
    if word_maps.shape[0] < 1:
        raise ValueError('localize needs at least one word map')
    if truth is not None:
        truth = _as_masks(truth, 'truth', word_maps.device)
        if truth.device != word_maps.device:
            raise RuntimeError('daam_amd: word maps and truth masks are on different devices')
        if tuple(truth.shape[1:]) != (out_h, out_w):
            raise ValueError(f'truth masks of {tuple(truth.shape[1:])} for an output of {(out_h, out_w)}: localize does not resize them')
    truth_blocks = [None] if truth is None else [truth[g:g + MAX_LOCATE_TRUTH] for g in range(0, truth.shape[0], MAX_LOCATE_TRUTH)]
    thr_blocks = [[float(t) for t in thr[k:k + MAX_LOCATE_THRESHOLDS]] for k in range(0, thr.size, MAX_LOCATE_THRESHOLDS)] or [[]]
    box_rows, peak_rows, value_rows, hit_rows, truth_boxes = [], [], [], [], []
    for i in range(0, word_maps.shape[0], MAX_LOCATE_WORDS):
        planes = word_maps[i:i + MAX_LOCATE_WORDS]
        # the first block of thresholds goes with the first block of truth masks; the other blocks of either go alone
        first = _launch_localize(planes, out_h, out_w, absolute, thr_blocks[0], truth_blocks[0])
        cols = [first[0]] + [_launch_localize(planes, out_h, out_w, absolute, ts, None)[0] for ts in thr_blocks[1:]]
        rest = [_launch_localize(planes, out_h, out_w, absolute, [], tb) for tb in truth_blocks[1:]]
        box_rows.append(torch.zeros(planes.shape[0], 0, 4, dtype=torch.int32, device=planes.device) if cols[0] is None else torch.cat(cols, dim=1))
        peak_rows.append(first[1])
        value_rows.append(first[2])
        if truth is not None:
            hit_rows.append(torch.cat([first[4]] + [r[4] for r in rest], dim=1))
            if not truth_boxes:
                truth_boxes = [first[3]] + [r[3] for r in rest]
    out = (torch.cat(box_rows), torch.cat(peak_rows), torch.cat(value_rows))
    if truth is None:
        return out + (None, None)
    return out + (torch.cat(truth_boxes), torch.cat(hit_rows) != 0)


MAX_COMPONENT_MASKS, MAX_COMPONENT_ROWS = 32, 65536      # limits of one daam_mask_components call (include/daam_components.h)
_KEEP_CODES = {None: 0, 0: 0, 'area': 1, 1: 1, 'largest': 2, 2: 2}


def _launch_components(masks: torch.Tensor, connectivity: int, min_area: int, keep: int, max_comp: int, labels: bool):
    """One ``daam_mask_components`` call: ``masks`` [M <= 32, H, W] uint8, contiguous -> ``(labels int32 [M, H, W] or None, counts
    int32 [M, 2], comps int32 [M, max_comp, 6], largest int32 [M, 6], kept uint8 [M, H, W] or None)``."""
    lib = nat.load_components()
    n, h, w = masks.shape
    dev = masks.device
    label_map = torch.empty(n, h, w, dtype=torch.int32, device=dev) if labels else None
    counts = torch.empty(n, 2, dtype=torch.int32, device=dev)
    comps = torch.empty(n, max_comp, 6, dtype=torch.int32, device=dev)
    largest = torch.empty(n, 6, dtype=torch.int32, device=dev)
    kept = torch.empty(n, h, w, dtype=torch.uint8, device=dev) if keep else None
    need = lib.daam_mask_components_workspace(n, h, w, max_comp)
    if not need:
        raise ValueError(f'mask_components of {n} masks at {h} x {w} with {max_comp} rows: out of range')
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        nat.check_components(lib.daam_mask_components(
            masks.data_ptr(), n, h, w, connectivity, min_area, keep, max_comp, label_map.data_ptr() if labels else None, counts.data_ptr(),
            comps.data_ptr() if max_comp else None, largest.data_ptr(), kept.data_ptr() if keep else None, ws.data_ptr(), need,
            torch.cuda.current_stream(dev).cuda_stream))
    return label_map, counts, comps, largest, kept


def mask_components(masks: torch.Tensor, connectivity: int = 8, min_area: int = 0, keep=None, max_components: int = 256,
                    labels: bool = True):
    """``daam_mask_components``: the connected components (``connectivity`` 4 or 8) of every mask of ``masks`` [M, H, W] (or [H, W];
    uint8 / bool as they are -- a byte != 0 is set --, other dtypes through ``!= 0``; CPU masks are moved to the device).  Returns
    device tensors ``(labels int32 [M, H, W] or None -- the rank of the pixel's component when a mask's components are sorted by their
    lowest row-major index, ``scipy.ndimage.label`` minus one; -1 on background --, counts int32 [M, 2] -- components; components of at
    least ``min_area`` pixels --, components int32 [M, max_components, 6] -- per rank the root, the area and x0 y0 x1 y1 inclusive;
    (-1, 0, W, H, -1, -1) past the last --, largest int32 [M, 6] -- the same columns for the component of the greatest area, the
    lowest root on a tie --, kept uint8 [M, H, W] or None)``.  ``keep``: ``None`` nothing, ``'area'`` the components of at least
    ``min_area`` pixels, ``'largest'`` the largest alone.  A mask with more components than ``max_components`` has its list cut
    and everything else exact.  More than 32 masks run in blocks that are concatenated on the device."""
    from .evaluate import _as_masks
    masks = _as_masks(masks, 'masks')
    if connectivity not in (4, 8):
        raise ValueError(f'connectivity {connectivity!r}: 4 or 8')
    if keep not in _KEEP_CODES:
        raise ValueError(f"keep {keep!r}: None, 'area' or 'largest'")
    min_area, max_components = int(min_area), int(max_components)
    if min_area < 0 or not 0 <= max_components <= MAX_COMPONENT_ROWS:
        raise ValueError(f'min_area {min_area} must be >= 0 and max_components {max_components} in 0..{MAX_COMPONENT_ROWS}')
    step = MAX_COMPONENT_MASKS
    parts = [_launch_components(masks[i:i + step], int(connectivity), min_area, _KEEP_CODES[keep], max_components, bool(labels))
             for i in range(0, masks.shape[0], step)]
    if len(parts) == 1:
        return parts[0]
    return tuple(None if col[0] is None else torch.cat(col) for col in zip(*parts))


MAX_REFINE_MAPS, MAX_REFINE_DILATIONS, MAX_REFINE_DILATION, MAX_REFINE_ITERATIONS = 32, 6, 64, 64   # include/daam_refine.h
REFINE_DILATIONS = (1, 2, 4, 8, 12, 24)


def _refine_dilations(dilations) -> Tuple[int, ...]:
    dil = tuple(int(d) for d in dilations)
    if not 1 <= len(dil) <= MAX_REFINE_DILATIONS or any(not 1 <= d <= MAX_REFINE_DILATION for d in dil) or \
            any(b <= a for a, b in zip(dil, dil[1:])):
        raise ValueError(f'dilations {dil!r}: 1..{MAX_REFINE_DILATIONS} strictly increasing integers within 1..{MAX_REFINE_DILATION}')
    return dil


def _image_bytes(image) -> torch.Tensor:
    """``image`` as uint8 [H, W, C], C 1 or 3, contiguous, on the device: a PIL image (modes other than L and RGB are converted to
    RGB) or a uint8 [H, W], [H, W, 1] or [H, W, 3] array or tensor (CPU ones are moved to the device)."""
    from .evaluate import _to_hip
    if hasattr(image, 'convert') and hasattr(image, 'mode'):
        image = torch.from_numpy(np.array(image if image.mode in ('L', 'RGB') else image.convert('RGB')))
    elif not isinstance(image, torch.Tensor):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if image.dtype != torch.uint8:
        raise RuntimeError(f'daam_amd: refinement reads a uint8 image, got {image.dtype}')
    if image.dim() == 2:
        image = image.unsqueeze(-1)
    if image.dim() != 3 or image.shape[2] not in (1, 3) or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f'image must be [H, W], [H, W, 1] or [H, W, 3], got {tuple(image.shape)}')
    return _to_hip(image, 'image').contiguous()


def refine_affinity(image, dilations=REFINE_DILATIONS, scale: float = 0.1) -> torch.Tensor:
    """``daam_refine_affinity``: the propagation weights of ``image`` (a PIL image, or a uint8 [H, W], [H, W, 1] or [H, W, 3] array or
    tensor; RGBA and other PIL modes are converted to RGB) as f32 [8 * len(dilations), H, W] on the device: per pixel the softmax over
    its 8 neighbours at every dilation of minus the mean absolute colour difference over ``scale`` times the local deviation
    (include/daam_refine.h).  They depend on the image alone: one call serves every word, threshold and ``refine_maps`` call."""
    lib = nat.load_refine()
    dil = _refine_dilations(dilations)
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError(f'scale {scale!r}: finite and > 0')
    pixels = _image_bytes(image)
    h, w, c = pixels.shape
    if not lib.daam_refine_weights_bytes(h, w, len(dil)):
        raise ValueError(f'an image of {h} x {w} with {len(dil)} dilations: out of range (fewer than 2^31 weights)')
    weights = torch.empty(8 * len(dil), h, w, dtype=torch.float32, device=pixels.device)
    with torch.cuda.device(pixels.device):
        nat.check_refine(lib.daam_refine_affinity(pixels.data_ptr(), h, w, c, (ctypes.c_int32 * len(dil))(*dil), len(dil), scale,
                                                  weights.data_ptr(), torch.cuda.current_stream(pixels.device).cuda_stream))
    return weights


def _launch_refine(weights: torch.Tensor, dil: Tuple[int, ...], maps: torch.Tensor, iterations: int, threshold: float, masks: bool,
                   labels: bool):
    """One ``daam_refine_apply`` call: ``maps`` [N <= 32, H, W] fp32, contiguous -> ``(refined f32 [N, H, W], masks uint8 [N, H, W] or
    None, labels uint8 [H, W] or None)``."""
    lib = nat.load_refine()
    n, h, w = maps.shape
    dev = maps.device
    refined = torch.empty(n, h, w, dtype=torch.float32, device=dev)
    mask_stack = torch.empty(n, h, w, dtype=torch.uint8, device=dev) if masks else None
    label_map = torch.empty(h, w, dtype=torch.uint8, device=dev) if labels else None
    need = lib.daam_refine_workspace(n, h, w)
    if not need:
        raise ValueError(f'refine_maps of {n} maps at {h} x {w}: out of range')
    ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        nat.check_refine(lib.daam_refine_apply(
            weights.data_ptr(), (ctypes.c_int32 * len(dil))(*dil), len(dil), maps.data_ptr(), n, h, w, iterations, threshold,
            refined.data_ptr(), mask_stack.data_ptr() if masks else None, label_map.data_ptr() if labels else None, ws.data_ptr(), need,
            torch.cuda.current_stream(dev).cuda_stream))
    return refined, mask_stack, label_map


def refine_maps(weights: torch.Tensor, dilations, maps: torch.Tensor, iterations: int = 10, threshold: float = 0.4, masks: bool = True,
                labels: bool = True):
    """``daam_refine_apply``: ``iterations`` rounds of ``m(p) <- sum_k weights[k](p) * m(q_k(p))`` on every map of ``maps``
    [N, H, W] fp32 on the device, with ``weights`` [8 * len(dilations), H, W] from ``refine_affinity`` of the same ``dilations``.
    Returns device tensors ``(refined f32 [N, H, W], masks uint8 [N, H, W] = refined > threshold or None, labels uint8 [H, W] -- the
    word with the largest refined value, the lowest index on a tie, 255 where none exceeds the threshold -- or None)``; masks and
    labels come out of the last iteration's launch.  More than 32 maps run in blocks that are concatenated on the device; a label
    map orders at most 32."""
    _check_maps(maps)
    dil = _refine_dilations(dilations)
    if weights.device != maps.device:
        raise RuntimeError('daam_amd: weights and maps are on different devices')
    if weights.dtype != torch.float32 or not weights.is_contiguous() or weights.dim() != 3:
        raise RuntimeError('daam_amd: refinement weights must be a contiguous fp32 [8 * dilations, H, W] tensor')
    if weights.shape[0] != 8 * len(dil):
        raise ValueError(f'{weights.shape[0]} weight planes for {len(dil)} dilations: {8 * len(dil)} are needed')
    if tuple(weights.shape[1:]) != tuple(maps.shape[1:]):
        raise ValueError(f'the weights are of an image of {weights.shape[1]} x {weights.shape[2]}, the maps are {maps.shape[1]} x {maps.shape[2]}')
    iterations, threshold = int(iterations), float(threshold)
    if not 0 <= iterations <= MAX_REFINE_ITERATIONS:
        raise ValueError(f'iterations {iterations}: 0..{MAX_REFINE_ITERATIONS}')
    if not math.isfinite(threshold):
        raise ValueError(f'threshold {threshold!r} is not finite')
    if maps.shape[0] < 1:
        raise ValueError('refine_maps needs at least one map')
    if labels and maps.shape[0] > MAX_REFINE_MAPS:
        raise ValueError(f'a label map orders at most {MAX_REFINE_MAPS} maps, got {maps.shape[0]}; pass labels=False')
    step = MAX_REFINE_MAPS
    parts = [_launch_refine(weights, dil, maps[i:i + step], iterations, threshold, bool(masks), bool(labels))
             for i in range(0, maps.shape[0], step)]
    if len(parts) == 1:
        return parts[0]
    return tuple(None if col[0] is None else torch.cat(col) for col in zip(*parts))


MAX_AFFINITY_CELLS, MAX_AFFINITY_SLICES, MAX_AFFINITY_MAPS, MAX_AFFINITY_ITERATIONS = 16384, 4096, 32, 16   # include/daam_self_affinity.h
AFFINITY_HEAD_DIMS = (40, 64, 80, 160)


def _check_on_device(query: torch.Tensor, key: torch.Tensor) -> None:
    if query.device.type != 'cuda' or key.device != query.device:
        raise RuntimeError('daam_amd: the self-attention affinity reads Q and K on the HIP device (no CPU fallback)')


class SelfAffinityState:
    """The self-attention affinity of one trace (include/daam_self_affinity.h): one f32 ``[P, P]`` tensor, P = h w cells
    of the heat map's grid, into which every tapped ``attn1`` call adds its head-summed ``softmax(Q K^T scale)``
    (``daam_self_affinity_accumulate``), the statistics workspace, and the counts of calls and slices.  Nothing is allocated before the
    first tapped call, whose launch overwrites the tensor (``accumulate = 0``)."""

    def __init__(self, h: int, w: int):
        self.grid = (int(h), int(w))
        self.cells = self.grid[0] * self.grid[1]
        if not 1 <= self.cells <= MAX_AFFINITY_CELLS:
            raise ValueError(f'a grid of {h} x {w} cells: the affinity takes 1..{MAX_AFFINITY_CELLS} cells')
        self.sums: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None
        self.calls = 0
        self.slices = 0

    def reset(self) -> None:
        """A new generation: the next tapped call overwrites the sums."""
        self.calls = self.slices = 0

    def tap(self, query: torch.Tensor, key: torch.Tensor, heads: int, scale: float, weight: float = 1.0) -> None:
        """``query`` / ``key``: what ``to_q`` / ``to_k`` gave, fp16 or bf16 ``[batch, P, heads * d]`` on the device, read in place
        through their strides."""
        lib = nat.load_self_affinity()
        _check_on_device(query, key)
        if query.dtype not in (torch.float16, torch.bfloat16) or key.dtype != query.dtype:
            raise RuntimeError(f'daam_amd: the self-attention affinity reads fp16 or bf16 Q and K, got {query.dtype} / {key.dtype}')
        if query.dim() != 3 or key.shape != query.shape or query.shape[1] != self.cells or query.shape[2] % heads:
            raise ValueError(f'self-affinity tap: Q {tuple(query.shape)} / K {tuple(key.shape)} on a grid of {self.cells} cells, {heads} heads')
        batch, cells, channels = query.shape
        d = channels // heads
        if d not in AFFINITY_HEAD_DIMS:
            raise ValueError(f'self-affinity tap: head dim {d}: one of {AFFINITY_HEAD_DIMS}')
        if query.stride(2) != 1:
            query = query.contiguous()
        if key.stride(2) != 1:
            key = key.contiguous()
        need = lib.daam_self_affinity_workspace(batch, heads, cells)
        if not need:
            raise ValueError(f'self-affinity tap: batch {batch} x {heads} heads: at most {MAX_AFFINITY_SLICES} slices')
        dev = query.device
        if self.sums is None or self.sums.device != dev:
            self.sums = torch.empty(cells, cells, dtype=torch.float32, device=dev)
            self.calls = self.slices = 0
        if self._ws is None or self._ws.device != dev or self._ws.numel() * 8 < need:
            self._ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            nat.check_self_affinity(lib.daam_self_affinity_accumulate(
                query.data_ptr(), key.data_ptr(), _DTYPE_CODE[query.dtype], batch, heads, cells, d, query.stride(0), d, query.stride(1),
                key.stride(0), d, key.stride(1), float(scale), float(weight), int(self.calls > 0), self.sums.data_ptr(), self._ws.data_ptr(),
                self._ws.numel() * 8, torch.cuda.current_stream(dev).cuda_stream))
        self.calls += 1
        self.slices += batch * heads


MAX_JOINT_CELLS, MAX_JOINT_TOKENS, MAX_JOINT_SLICES = 16384, 512, 4096     # include/daam_joint_tap.h
JOINT_HEAD_DIMS = (64, 128)


class JointTapState:
    """The heat-map sums of one trace of an MMDiT pipeline (include/daam_joint_tap.h): one f32 ``[T, h w]`` tensor (with
    ``per_head`` ``[heads, T, h w]``) into which every tapped joint-attention call adds the text columns of its softmax over text and
    image keys (``daam_joint_tap_accumulate``), the statistics workspace, and the counts of calls and slices.  Nothing is allocated
    before the first tapped call, whose launch overwrites the tensor (``accumulate = 0``)."""

    def __init__(self, h: int, w: int, tokens: int, per_head: bool = False):
        self.grid = (int(h), int(w))
        self.cells = self.grid[0] * self.grid[1]
        self.tokens = int(tokens)
        self.per_head = bool(per_head)
        if not 1 <= self.cells <= MAX_JOINT_CELLS:
            raise ValueError(f'a grid of {h} x {w} cells: the joint tap takes 1..{MAX_JOINT_CELLS} cells')
        if not 1 <= self.tokens <= MAX_JOINT_TOKENS:
            raise ValueError(f'{tokens} text tokens: the joint tap takes 1..{MAX_JOINT_TOKENS}')
        self.sums: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None           # this state's own workspace: what `tap` has the library write
        self._stats: Optional[torch.Tensor] = None        # the statistics of the last tapped call: `_ws`, or a view that was given
        self.heads = 0
        self.calls = 0
        self.slices = 0

    def reset(self) -> None:
        """A new generation: the next tapped call overwrites the sums."""
        self.calls = self.slices = 0

    def _checked(self, q, k_txt, k_img, heads: int):
        """What ``tap`` and ``tap_from_stats`` (``k_img`` None) hold their tensors to: ``(tensors with a unit last stride, batch, d)``."""
        given = [t for t in (q, k_txt, k_img) if t is not None]
        for t in given[1:]:
            _check_on_device(q, t)
        if q.dtype not in (torch.float16, torch.bfloat16) or any(t.dtype != q.dtype for t in given):
            raise RuntimeError(f'daam_amd: the joint tap reads fp16 or bf16 Q and K, got {" / ".join(str(t.dtype) for t in given)}')
        if (any(t.dim() != 3 for t in given) or q.shape[1] != self.cells or k_txt.shape[1] != self.tokens
                or any(t.shape[0] != q.shape[0] or t.shape[2] != q.shape[2] for t in given) or q.shape[2] % heads
                or (k_img is not None and k_img.shape[1] > MAX_JOINT_CELLS)):
            shapes = ' / '.join(f'{name} {tuple(t.shape)}' for name, t in zip(('Q', 'text K', 'image K'), given))
            raise ValueError(f'joint tap: {shapes} on a grid of {self.cells} cells with {self.tokens} tokens, {heads} heads')
        d = q.shape[2] // heads
        if d not in JOINT_HEAD_DIMS:
            raise ValueError(f'joint tap: head dim {d}: one of {JOINT_HEAD_DIMS}')
        if self.per_head and self.sums is not None and self.calls and heads != self.heads:
            raise ValueError(f'joint tap: {heads} heads after calls with {self.heads}: per-head planes need one head count')
        return [t if t.stride(2) == 1 else t.contiguous() for t in given], q.shape[0], d

    def _sums_on(self, dev, heads: int) -> None:
        """The sums of this call: allocated anew (and the counts reset) where there are none on ``dev`` in this call's shape."""
        shape = (heads, self.tokens, self.cells) if self.per_head else (self.tokens, self.cells)
        if self.sums is None or self.sums.device != dev or self.sums.shape != shape:
            self.sums = torch.empty(shape, dtype=torch.float32, device=dev)
            self.calls = self.slices = 0
        self.heads = heads

    def tap(self, q: torch.Tensor, k_txt: torch.Tensor, k_img: torch.Tensor, heads: int, scale: float, weight: float = 1.0) -> None:
        """``q`` / ``k_txt`` / ``k_img``: what the projections (and their norms) gave, fp16 or bf16 ``[batch, rows, heads * d]`` on the
        device with ``rows`` = cells / tokens / image keys, read in place through their strides."""
        lib = nat.load_joint()
        (q, k_txt, k_img), batch, d = self._checked(q, k_txt, k_img, heads)
        cells = self.cells
        need = lib.daam_joint_tap_workspace(batch, heads, cells)
        if not need:
            raise ValueError(f'joint tap: batch {batch} x {heads} heads: at most {MAX_JOINT_SLICES} slices')
        dev = q.device
        self._sums_on(dev, heads)
        if self._ws is None or self._ws.device != dev or self._ws.numel() * 8 < need:
            self._ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            nat.check_joint(lib.daam_joint_tap_accumulate(
                q.data_ptr(), k_txt.data_ptr(), k_img.data_ptr() if k_img.shape[1] else None, _DTYPE_CODE[q.dtype], batch, heads, cells,
                self.tokens, k_img.shape[1], d, q.stride(0), d, q.stride(1), k_txt.stride(0), d, k_txt.stride(1), k_img.stride(0), d,
                k_img.stride(1), float(scale), float(weight), int(self.calls > 0), self.sums.data_ptr(),
                self.tokens * cells if self.per_head else 0, self._ws.data_ptr(), self._ws.numel() * 8,
                torch.cuda.current_stream(dev).cuda_stream))
        self._stats = self._ws
        self.calls += 1
        self.slices += batch * heads

    def tap_from_stats(self, q: torch.Tensor, k_txt: torch.Tensor, heads: int, scale: float, stats: torch.Tensor, weight: float = 1.0) -> None:
        """The text columns from statistics that are there already (``daam_joint_attend_text``, include/daam_joint_attend.h): ``q`` /
        ``k_txt`` as ``tap`` takes them (and holds them to: the same checks, the same errors), ``stats`` a view of
        ``JointAttendState.forward``'s statistics that begins at the first slice of ``q``'s first batch entry.  Allocation, bookkeeping
        and the first-call-overwrites rule are those of ``tap``; ``self.stats`` becomes ``stats``, so that the affinity reads the same
        thing.  The view is only read and is never taken for this state's own workspace."""
        lib = _load_joint_attend()
        (q, k_txt), batch, d = self._checked(q, k_txt, None, heads)
        cells = self.cells
        need = lib.daam_joint_attend_stats_bytes(batch, heads, cells)
        if not need:
            raise ValueError(f'joint tap: batch {batch} x {heads} heads: at most {MAX_JOINT_SLICES} slices')
        if stats is None or stats.device != q.device or stats.numel() * stats.element_size() < need:
            raise ValueError(f'joint tap: the statistics of {batch * heads} slices of {cells} rows take {need} bytes on the device of Q: '
                             f'pass the statistics JointAttendState.forward returned, offset to the first batch entry of Q')
        dev = q.device
        self._sums_on(dev, heads)
        with torch.cuda.device(dev):
            nat.check_joint_attend(lib.daam_joint_attend_text(
                q.data_ptr(), k_txt.data_ptr(), stats.data_ptr(), stats.numel() * stats.element_size(), _DTYPE_CODE[q.dtype], batch, heads,
                cells, self.tokens, d, q.stride(0), d, q.stride(1), k_txt.stride(0), d, k_txt.stride(1), float(scale), float(weight),
                int(self.calls > 0), self.sums.data_ptr(), self.tokens * cells if self.per_head else 0,
                torch.cuda.current_stream(dev).cuda_stream))
        self._stats = stats
        self.calls += 1
        self.slices += batch * heads

    @property
    def stats(self) -> Optional[torch.Tensor]:
        """The statistics of the last tapped call, read-only to callers: the workspace ``tap`` wrote, or the view ``tap_from_stats`` was
        given.  Per slice and query row the ``float2`` ``(-(m c), 1 / l)`` of the joint softmax, slices ``pad128(cells)`` rows apart
        (the layout include/daam_joint_affinity.h states).  ``None`` before a tap."""
        return self._stats


JOINT_TAP_STATS_ABI = 1                             # the daam_joint_tap ABI whose workspace layout daam_joint_affinity.h reads
_joint_affinity_checked = False


def _load_joint_affinity():
    """``nat.load_joint_affinity()``; the first call also holds ``libdaam_joint.so`` to the ABI whose workspace holds the statistics in
    the layout the affinity reads."""
    global _joint_affinity_checked
    lib = nat.load_joint_affinity()
    if not _joint_affinity_checked:
        tap_abi = nat.load_joint().daam_joint_tap_abi_version()
        if tap_abi != JOINT_TAP_STATS_ABI:
            raise RuntimeError(f'daam_amd: the joint affinity reads the statistics of daam_joint_tap ABI {JOINT_TAP_STATS_ABI}, '
                               f'libdaam_joint.so reports {tap_abi}; rebuild')
        _joint_affinity_checked = True
    return lib


class JointAffinityState:
    """The image-to-image affinity of one trace of an MMDiT / FLUX pipeline (include/daam_joint_affinity.h): one f32
    ``[P, P]`` tensor, P = h w cells, into which every tapped joint-attention call adds the image columns of its softmax over text and
    image keys (``daam_joint_affinity_accumulate``), and the counts of calls and slices.  It holds no statistics: each ``tap`` is fed
    those the joint tap of the same call has just written (``JointTapState.stats``).  Nothing is allocated before the first tapped
    call, whose launch overwrites the tensor (``accumulate = 0``).  A row of the tensor sums to ``slices`` minus the mass the cell gave
    to the text keys."""

    def __init__(self, h: int, w: int):
        self.grid = (int(h), int(w))
        self.cells = self.grid[0] * self.grid[1]
        if not 1 <= self.cells <= MAX_JOINT_CELLS:
            raise ValueError(f'a grid of {h} x {w} cells: the joint affinity takes 1..{MAX_JOINT_CELLS} cells')
        self.sums: Optional[torch.Tensor] = None
        self.calls = 0
        self.slices = 0

    def reset(self) -> None:
        """A new generation: the next tapped call overwrites the sums."""
        self.calls = self.slices = 0

    def tap(self, q: torch.Tensor, k_img: torch.Tensor, heads: int, scale: float, stats: torch.Tensor, weight: float = 1.0) -> None:
        """``q`` / ``k_img``: what ``JointTapState.tap`` was just given, fp16 or bf16 ``[batch, cells, heads * d]`` on the device, read
        in place through their strides; ``stats``: that state's ``stats`` after the call; ``scale``: the scale of that call."""
        lib = _load_joint_affinity()
        _check_on_device(q, k_img)
        if q.dtype not in (torch.float16, torch.bfloat16) or k_img.dtype != q.dtype:
            raise RuntimeError(f'daam_amd: the joint affinity reads fp16 or bf16 Q and K, got {q.dtype} / {k_img.dtype}')
        if (q.dim() != 3 or k_img.dim() != 3 or q.shape[1] != self.cells or k_img.shape[1] != self.cells or k_img.shape[0] != q.shape[0]
                or k_img.shape[2] != q.shape[2] or q.shape[2] % heads):
            raise ValueError(f'joint affinity tap: Q {tuple(q.shape)} / image K {tuple(k_img.shape)} on a grid of {self.cells} cells '
                             f'(the affinity is square), {heads} heads')
        batch, cells, channels = q.shape
        d = channels // heads
        if d not in JOINT_HEAD_DIMS:
            raise ValueError(f'joint affinity tap: head dim {d}: one of {JOINT_HEAD_DIMS}')
        q, k_img = (t if t.stride(2) == 1 else t.contiguous() for t in (q, k_img))
        need = lib.daam_joint_affinity_stats_bytes(batch, heads, cells)
        if not need:
            raise ValueError(f'joint affinity tap: batch {batch} x {heads} heads: at most {MAX_JOINT_SLICES} slices')
        if stats is None or stats.device != q.device or stats.numel() * stats.element_size() < need:
            raise ValueError(f'joint affinity tap: the statistics of {batch * heads} slices of {cells} rows take {need} bytes on the '
                             f'device of Q: pass JointTapState.stats of the same call')
        dev = q.device
        if self.sums is None or self.sums.device != dev:
            self.sums = torch.empty(cells, cells, dtype=torch.float32, device=dev)
            self.calls = self.slices = 0
        with torch.cuda.device(dev):
            nat.check_joint_affinity(lib.daam_joint_affinity_accumulate(
                q.data_ptr(), k_img.data_ptr(), stats.data_ptr(), stats.numel() * stats.element_size(), _DTYPE_CODE[q.dtype], batch, heads,
                cells, cells, d, q.stride(0), d, q.stride(1), k_img.stride(0), d, k_img.stride(1), float(scale), float(weight),
                int(self.calls > 0), self.sums.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        self.calls += 1
        self.slices += batch * heads


JOINT_ATTEND_ABI = 1                                # include/daam_joint_attend.h


def _load_joint_attend():
    """``nat.load_joint_attend()``, held to the ABI this module's calls are written for."""
    lib = nat.load_joint_attend()
    abi = lib.daam_joint_attend_abi_version()
    if abi != JOINT_ATTEND_ABI:
        raise RuntimeError(f'daam_amd: libdaam_jointattend.so reports ABI {abi}, this module calls ABI {JOINT_ATTEND_ABI}; rebuild')
    return lib


def pad128(rows: int) -> int:
    """Rows of a slice's statistics (include/daam_joint_affinity.h)."""
    return -(-int(rows) // 128) * 128


class JointAttendState:
    """The joint attention of an MMDiT block computed by the library (include/daam_joint_attend.h): softmax(Q K^T) V for
    the image and the text queries over text and image keys, with the image rows' softmax statistics left behind by the same walk.
    It holds the statistics buffer between calls and nothing else; the library is loaded by the first ``forward``."""

    def __init__(self):
        self._stats: Optional[torch.Tensor] = None
        self.calls = 0

    def forward(self, q_img: torch.Tensor, k_img: torch.Tensor, v_img: torch.Tensor, q_txt: torch.Tensor, k_txt: torch.Tensor,
                v_txt: torch.Tensor, heads: int, scale: float):
        """Six fp16 or bf16 ``[B, rows, heads * d]`` tensors as the projections (and their norms) gave them, ``rows`` = P for the
        image three and T for the text three, read in place through their strides.  Returns ``(out_img [B, P, heads d],
        out_txt [B, T, heads d], stats)``; ``stats`` is an int64 view of ``B * heads * pad128(P)`` ``float2`` pairs, overwritten by
        the next ``forward``."""
        lib = _load_joint_attend()
        img, txt = (q_img, k_img, v_img), (q_txt, k_txt, v_txt)
        for t in img + txt:
            _check_on_device(q_img, t)
        if q_img.dtype not in (torch.float16, torch.bfloat16) or any(t.dtype != q_img.dtype for t in img + txt):
            raise ValueError(f'joint attend: fp16 or bf16 Q, K and V of one dtype, got {[str(t.dtype) for t in img + txt]}')
        if (any(t.dim() != 3 for t in img + txt) or any(t.shape != q_img.shape for t in img) or any(t.shape != q_txt.shape for t in txt)
                or q_txt.shape[0] != q_img.shape[0] or q_txt.shape[2] != q_img.shape[2] or q_img.shape[2] % heads
                or not 1 <= q_img.shape[1] <= MAX_JOINT_CELLS or not 1 <= q_txt.shape[1] <= MAX_JOINT_TOKENS):
            raise ValueError(f'joint attend: image Q / K / V {[tuple(t.shape) for t in img]}, text Q / K / V {[tuple(t.shape) for t in txt]}, '
                             f'{heads} heads: [B, 1..{MAX_JOINT_CELLS}, heads d] and [B, 1..{MAX_JOINT_TOKENS}, heads d]')
        batch, cells, channels = q_img.shape
        tokens = q_txt.shape[1]
        d = channels // heads
        if d not in JOINT_HEAD_DIMS:
            raise ValueError(f'joint attend: head dim {d}: one of {JOINT_HEAD_DIMS}')
        need = lib.daam_joint_attend_stats_bytes(batch, heads, cells)
        if not need:
            raise ValueError(f'joint attend: batch {batch} x {heads} heads: at most {MAX_JOINT_SLICES} slices')
        img = tuple(t if t.stride(2) == 1 else t.contiguous() for t in img)
        txt = tuple(t if t.stride(2) == 1 else t.contiguous() for t in txt)
        dev = q_img.device
        out_img = torch.empty(batch, cells, channels, dtype=q_img.dtype, device=dev)
        out_txt = torch.empty(batch, tokens, channels, dtype=q_img.dtype, device=dev)
        if self._stats is None or self._stats.device != dev or self._stats.numel() * 8 != need:
            self._stats = torch.empty(need // 8, dtype=torch.int64, device=dev)
        strides = lambda ts: (ctypes.c_int64 * (3 * len(ts)))(*[v for t in ts for v in (t.stride(0), d, t.stride(1))])
        with torch.cuda.device(dev):
            nat.check_joint_attend(lib.daam_joint_attend_forward(
                *[t.data_ptr() for t in img + txt], out_img.data_ptr(), out_txt.data_ptr(), _DTYPE_CODE[q_img.dtype], batch, heads, cells,
                tokens, d, strides(img), strides(txt), strides((out_img, out_txt)), float(scale), self._stats.data_ptr(), need,
                torch.cuda.current_stream(dev).cuda_stream))
        self.calls += 1
        return out_img, out_txt, self._stats


MAX_ROPE_JOBS, MAX_ROPE_ROWS, MAX_ROPE_SLICES = 4, 16896, 4096                 # include/daam_rope.h
ROPE_HEAD_DIMS = (64, 128)


class RopeTable:
    """The cos / sin tables of a generation in the form ``rope_apply`` reads: f32, ``stride(-1) == 1``, rows a multiple of 4 floats
    apart, 16-byte aligned.  A table that is so already is handed back as it is; anything else goes through ``.float().contiguous()``
    ONCE and is found again by its ``data_ptr`` (the pipeline passes the same table to every block of every step).  The source is
    kept alive beside its copy so that its address cannot be given to another tensor; ``reset()`` (a new generation) forgets both."""

    def __init__(self):
        self._cache: Dict[Tuple, Tuple[torch.Tensor, torch.Tensor]] = {}

    def reset(self) -> None:
        self._cache.clear()

    def __len__(self) -> int:
        return len(self._cache)

    @staticmethod
    def fits(table: torch.Tensor) -> bool:
        return (table.dtype == torch.float32 and table.dim() == 2 and table.stride(1) == 1 and table.stride(0) % 4 == 0
                and table.stride(0) >= table.shape[1] and table.data_ptr() % 16 == 0)

    def get(self, table: torch.Tensor) -> torch.Tensor:
        if table.dim() != 2:
            raise ValueError(f'rope table: {tuple(table.shape)}: [rows, d]')
        if self.fits(table):
            return table
        key = (table.data_ptr(), table.dtype, tuple(table.shape), table.stride(), table.device)
        hit = self._cache.get(key)
        if hit is None:
            hit = self._cache[key] = (table, table.float().contiguous())
        return hit[1]


def rope_apply(jobs: Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, int]], d: int) -> None:
    """One ``daam_rope_apply`` launch (include/daam_rope.h) on the current stream.  A job is ``(x, out, cos, sin, heads)``:
    ``x`` fp16 or bf16 ``[batch, rows, heads * d]`` on the device -- what a projection gave, or a row range of it --, ``out`` a view of
    the same shape and dtype that does not overlap it, ``cos`` / ``sin`` f32 ``[rows, d]`` with ``stride(-1) == 1`` (``RopeTable.get``
    of the pipeline's table, sliced to the job's rows).  Strides are read off the tensors; the head stride is ``d``."""
    lib = nat.load_rope()
    if not 1 <= len(jobs) <= MAX_ROPE_JOBS:
        raise ValueError(f'rope_apply: {len(jobs)} jobs: 1..{MAX_ROPE_JOBS}')
    if d not in ROPE_HEAD_DIMS:
        raise ValueError(f'rope_apply: head dim {d}: one of {ROPE_HEAD_DIMS}')
    first = jobs[0][0]
    if first.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError(f'daam_amd: rope_apply rotates fp16 or bf16 tensors, got {first.dtype}')
    table = (nat.RopeJob * len(jobs))()
    for n, (x, out, cos, sin, heads) in enumerate(jobs):
        for t in (out, cos, sin):
            _check_on_device(x, t)
        if x.device != first.device:
            raise RuntimeError('daam_amd: rope_apply: the jobs of one launch live on one device')
        if x.dtype != first.dtype or out.dtype != x.dtype:
            raise RuntimeError(f'daam_amd: rope_apply: job {n}: x {x.dtype} / out {out.dtype} in a launch of {first.dtype}')
        if x.dim() != 3 or out.shape != x.shape or heads < 1 or x.shape[2] != heads * d or x.stride(2) != 1 or out.stride(2) != 1:
            raise ValueError(f'rope_apply: job {n}: x {tuple(x.shape)} / out {tuple(out.shape)}: [batch, rows, {heads} heads * {d}], channels contiguous')
        batch, rows, _ = x.shape
        if not 1 <= rows <= MAX_ROPE_ROWS or batch < 1 or batch * heads > MAX_ROPE_SLICES:
            raise ValueError(f'rope_apply: job {n}: {rows} rows (1..{MAX_ROPE_ROWS}), batch {batch} x {heads} heads (at most {MAX_ROPE_SLICES} slices)')
        for name, t in (('cos', cos), ('sin', sin)):
            if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (rows, d) or t.stride(1) != 1:
                raise ValueError(f'rope_apply: job {n}: {name} {t.dtype} {tuple(t.shape)}: f32 [{rows}, {d}] with stride(-1) == 1 (RopeTable.get)')
        if rows > 1 and cos.stride(0) != sin.stride(0):
            raise ValueError(f'rope_apply: job {n}: cos rows {cos.stride(0)} floats apart, sin rows {sin.stride(0)}: one table_stride')
        table[n] = nat.RopeJob(x.data_ptr(), out.data_ptr(), cos.data_ptr(), sin.data_ptr(), batch, heads, rows,
                               x.stride(0) if batch > 1 else 0, x.stride(1) if rows > 1 else d * heads, d,
                               out.stride(0) if batch > 1 else 0, out.stride(1) if rows > 1 else d * heads, d,
                               cos.stride(0) if rows > 1 else d)
    with _device_guard(first.device):
        nat.check_rope(lib.daam_rope_apply(table, len(jobs), _DTYPE_CODE[first.dtype], d, torch.cuda.current_stream(first.device).cuda_stream))


def _launch_propagate(sums: torch.Tensor, maps: torch.Tensor, iterations: int) -> torch.Tensor:
    """One ``daam_self_affinity_propagate`` call: ``maps`` [N <= 32, P] fp32, contiguous -> f32 [N, P]."""
    lib = nat.load_self_affinity()
    n, cells = maps.shape
    dev = maps.device
    need = _PROPAGATE_NEED.get((n, cells))
    if need is None:
        need = _PROPAGATE_NEED[(n, cells)] = lib.daam_self_affinity_propagate_workspace(n, cells)
    if not need:
        raise ValueError(f'affinity_propagate of {n} maps of {cells} cells: out of range')
    # one allocation: the result, then the workspace behind it (a few hundred KB that live as long as the result does)
    buf = torch.empty(n * cells + need // 4, dtype=torch.float32, device=dev)
    out = buf.data_ptr()
    with _device_guard(dev):
        nat.check_self_affinity(lib.daam_self_affinity_propagate(sums.data_ptr(), cells, maps.data_ptr(), n, iterations, out, out + 4 * n * cells,
                                                                 need, torch.cuda.current_stream(dev).cuda_stream))
    return buf[:n * cells].view(n, cells)


_PROPAGATE_NEED: Dict[Tuple[int, int], int] = {}     # (maps, cells) -> daam_self_affinity_propagate_workspace, a pure function of them


def _device_guard(dev: torch.device):
    """``torch.cuda.device(dev)``, or nothing where ``dev`` is the current device already (the common case: entering the context costs
    several microseconds of a call that takes tens)."""
    if dev.index is None or dev.index == torch.cuda.current_device():
        return contextlib.nullcontext()
    return torch.cuda.device(dev)


def affinity_propagate(sums: torch.Tensor, maps: torch.Tensor, iterations: int = 1) -> torch.Tensor:
    """``daam_self_affinity_propagate``: ``iterations`` rounds of ``m(i) <- sum_j sums[i][j] m(j) / sum_j sums[i][j]`` on every map of
    ``maps`` [N, h, w] fp32 on the device, ``sums`` the fp32 [h w, h w] affinity (entries finite and >= 0).  Returns f32 [N, h, w]; more
    than 32 maps run in blocks that are concatenated on the device."""
    _check_maps(maps)
    if sums.device != maps.device:
        raise RuntimeError('daam_amd: the affinity and the maps are on different devices')
    if sums.dtype != torch.float32 or not sums.is_contiguous() or sums.dim() != 2 or sums.shape[0] != sums.shape[1]:
        raise RuntimeError('daam_amd: the affinity must be a contiguous fp32 [P, P] tensor')
    n, h, w = maps.shape
    if h * w != sums.shape[0]:
        raise ValueError(f'the affinity is of {sums.shape[0]} cells, the maps are {h} x {w}')
    iterations = int(iterations)
    if not 0 <= iterations <= MAX_AFFINITY_ITERATIONS:
        raise ValueError(f'iterations {iterations}: 0..{MAX_AFFINITY_ITERATIONS}')
    if n < 1:
        raise ValueError('affinity_propagate needs at least one map')
    flat = maps.reshape(n, h * w)
    parts = [_launch_propagate(sums, flat[i:i + MAX_AFFINITY_MAPS], iterations) for i in range(0, n, MAX_AFFINITY_MAPS)]
    return (parts[0] if len(parts) == 1 else torch.cat(parts)).reshape(n, h, w)


MAX_DISCOVER_ROWS, MAX_DISCOVER_CELLS, MAX_DISCOVER_GROUPS = 16384, 16384, 1024            # include/daam_discover.h
MAX_DISCOVER_PROPOSALS, MAX_DISCOVER_GRID, MAX_DISCOVER_OUT = 255, 128, 2048


def _check_discover(name: str, t: torch.Tensor, dtype: torch.dtype, dims: int, like: Optional[torch.Tensor] = None) -> None:
    """What every operand of the discovery launchers owes: the dtype, the rank, the HIP device (that of ``like``)."""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dims:
        got = f'{t.dtype} {tuple(t.shape)}' if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f'{name}: {got}: a {dtype} tensor of {dims} dimensions')
    _check_discover_device(t, like)


def _check_discover_device(t: torch.Tensor, like: Optional[torch.Tensor]) -> None:
    if t.device.type != 'cuda' or (like is not None and t.device != like.device):
        raise RuntimeError('daam_amd: the discovery passes read their operands on one HIP device (no CPU fallback)')


def _stream_of(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def discover_prepare(src: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``daam_discover_prepare`` (include/daam_discover.h): ``src`` f32 [R, N] on the device with ``stride(1) == 1`` (rows
    may be further apart than N) -> ``(P, L)``, f32 [R, N] each: the rows divided by their sums, and ``logf(max(P, 2^-120))``.  A row
    whose sum is 0 or not finite gives ``P = 0``.  ``out``: the caller's own contiguous ``(P, L)`` to be overwritten."""
    lib = nat.load_discover()
    _check_discover('discover_prepare: src', src, torch.float32, 2)
    rows, n = src.shape
    if not (1 <= rows <= MAX_DISCOVER_ROWS and 1 <= n <= MAX_DISCOVER_CELLS):
        raise ValueError(f'discover_prepare: src {tuple(src.shape)}: 1..{MAX_DISCOVER_ROWS} rows of 1..{MAX_DISCOVER_CELLS} cells')
    if (n > 1 and src.stride(1) != 1) or (rows > 1 and src.stride(0) < n):
        raise ValueError(f'discover_prepare: src strides {src.stride()}: cells contiguous, rows at least {n} apart')
    p, l = out if out is not None else (torch.empty(rows, n, dtype=torch.float32, device=src.device) for _ in range(2))
    for name, t in (('P', p), ('L', l)):
        _check_discover(f'discover_prepare: {name}', t, torch.float32, 2, src)
        if tuple(t.shape) != (rows, n) or not t.is_contiguous():
            raise ValueError(f'discover_prepare: {name} {tuple(t.shape)}: contiguous [{rows}, {n}]')
    with torch.cuda.device(src.device):
        nat.check_discover(lib.daam_discover_prepare(src.data_ptr(), src.stride(0) if rows > 1 else n, rows, n, p.data_ptr(), l.data_ptr(),
                                                     _stream_of(src.device)))
    return p, l


def discover_pair_kl(pa: torch.Tensor, la: torch.Tensor, pb: torch.Tensor, lb: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``daam_discover_pair_kl``: ``D[a][b] = 1/2 sum_j (pa[a][j] - pb[b][j]) (la[a][j] - lb[b][j])``, f32 [A, B], of contiguous f32
    ``pa`` / ``la`` [A, N] and ``pb`` / ``lb`` [B, N] on the device (``discover_prepare`` gives such pairs)."""
    lib = nat.load_discover()
    for name, t in (('pa', pa), ('la', la), ('pb', pb), ('lb', lb)):
        _check_discover(f'discover_pair_kl: {name}', t, torch.float32, 2, pa)
        if not t.is_contiguous():
            raise ValueError(f'discover_pair_kl: {name} must be contiguous')
    (a, n), (b, nb) = pa.shape, pb.shape
    if la.shape != pa.shape or lb.shape != pb.shape or nb != n:
        raise ValueError(f'discover_pair_kl: pa {tuple(pa.shape)} / la {tuple(la.shape)} / pb {tuple(pb.shape)} / lb {tuple(lb.shape)}: [A, N], [A, N], [B, N], [B, N]')
    if not (1 <= a <= MAX_DISCOVER_ROWS and 1 <= b <= MAX_DISCOVER_ROWS and 1 <= n <= MAX_DISCOVER_CELLS):
        raise ValueError(f'discover_pair_kl: {a} x {b} rows of {n} cells: 1..{MAX_DISCOVER_ROWS} rows, 1..{MAX_DISCOVER_CELLS} cells')
    d = out if out is not None else torch.empty(a, b, dtype=torch.float32, device=pa.device)
    _check_discover('discover_pair_kl: out', d, torch.float32, 2, pa)
    if tuple(d.shape) != (a, b) or not d.is_contiguous():
        raise ValueError(f'discover_pair_kl: out {tuple(d.shape)}: contiguous [{a}, {b}]')
    with torch.cuda.device(pa.device):
        nat.check_discover(lib.daam_discover_pair_kl(pa.data_ptr(), la.data_ptr(), a, pb.data_ptr(), lb.data_ptr(), b, n, d.data_ptr(),
                                                     _stream_of(pa.device)))
    return d


def discover_merge(p: torch.Tensor, member: torch.Tensor, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``daam_discover_merge``: ``p`` f32 [R, N] and ``member`` uint8 [K, R], contiguous on the device -> ``(out, cnt)``: f32 [K, N],
    the mean of the rows ``r`` with ``member[k][r] != 0`` added in ascending ``r`` (zeros where there is none), and int32 [K], their
    number."""
    lib = nat.load_discover()
    _check_discover('discover_merge: p', p, torch.float32, 2)
    _check_discover('discover_merge: member', member, torch.uint8, 2, p)
    (rows, n), k = p.shape, member.shape[0]
    if member.shape[1] != rows or not p.is_contiguous() or not member.is_contiguous():
        raise ValueError(f'discover_merge: p {tuple(p.shape)} / member {tuple(member.shape)}: contiguous [R, N] and [K, R]')
    if not (1 <= rows <= MAX_DISCOVER_ROWS and 1 <= n <= MAX_DISCOVER_CELLS and 1 <= k <= MAX_DISCOVER_GROUPS):
        raise ValueError(f'discover_merge: {rows} rows of {n} cells into {k} groups: 1..{MAX_DISCOVER_ROWS}, 1..{MAX_DISCOVER_CELLS}, 1..{MAX_DISCOVER_GROUPS}')
    merged, cnt = out if out is not None else (torch.empty(k, n, dtype=torch.float32, device=p.device),
                                               torch.empty(k, dtype=torch.int32, device=p.device))
    _check_discover('discover_merge: out', merged, torch.float32, 2, p)
    _check_discover('discover_merge: cnt', cnt, torch.int32, 1, p)
    if tuple(merged.shape) != (k, n) or cnt.shape[0] != k or not merged.is_contiguous() or not cnt.is_contiguous():
        raise ValueError(f'discover_merge: out {tuple(merged.shape)} / cnt {tuple(cnt.shape)}: contiguous [{k}, {n}] and [{k}]')
    with torch.cuda.device(p.device):
        nat.check_discover(lib.daam_discover_merge(p.data_ptr(), rows, n, member.data_ptr(), k, merged.data_ptr(), cnt.data_ptr(),
                                                   _stream_of(p.device)))
    return merged, cnt


def discover_labels(props: torch.Tensor, out_h: int, out_w: int, values: bool = False):
    """``daam_discover_labels``: ``props`` f32 [K, h, w], contiguous on the device -> uint8 [out_h, out_w], at every pixel the lowest
    index among the largest bilinearly resized proposals (``F.interpolate(mode='bilinear', align_corners=False)``; a plain argmax when
    the size is the grid's).  ``values=True``: ``(labels, f32 [out_h, out_w])`` with the winner's resized value."""
    lib = nat.load_discover()
    _check_discover('discover_labels: props', props, torch.float32, 3)
    k, h, w = props.shape
    out_h, out_w = int(out_h), int(out_w)
    if not props.is_contiguous() or not (1 <= k <= MAX_DISCOVER_PROPOSALS and 1 <= h <= MAX_DISCOVER_GRID and 1 <= w <= MAX_DISCOVER_GRID):
        raise ValueError(f'discover_labels: props {tuple(props.shape)}: contiguous, 1..{MAX_DISCOVER_PROPOSALS} proposals on a grid of 1..{MAX_DISCOVER_GRID} cells a side')
    if not (1 <= out_h <= MAX_DISCOVER_OUT and 1 <= out_w <= MAX_DISCOVER_OUT):
        raise ValueError(f'discover_labels: output {out_h} x {out_w}: 1..{MAX_DISCOVER_OUT} a side')
    labels = torch.empty(out_h, out_w, dtype=torch.uint8, device=props.device)
    vals = torch.empty(out_h, out_w, dtype=torch.float32, device=props.device) if values else None
    with torch.cuda.device(props.device):
        nat.check_discover(lib.daam_discover_labels(props.data_ptr(), k, h, w, out_h, out_w, labels.data_ptr(),
                                                    vals.data_ptr() if values else None, _stream_of(props.device)))
    return (labels, vals) if values else labels


def _check_maps(maps: torch.Tensor) -> None:
    if maps.device.type != 'cuda':
        raise RuntimeError('daam_amd: heat maps must live on the HIP device (no CPU fallback)')
    if maps.dtype != torch.float32 or not maps.is_contiguous() or maps.dim() != 3:
        raise RuntimeError('daam_amd: heat maps must be a contiguous fp32 [rows, h, w] tensor')


MAX_BLEND_SETS = 8                                # limit of one daam_key_blend call (include/daam_analysis.h)
MAX_REGION_MASKS = 32                             # limit of one daam_region_scores call (include/daam_hip.h)


def _check_map_sets(maps: torch.Tensor) -> torch.Tensor:
    """``[rows, h, w]`` or ``[G, rows, h, w]`` -> the 4-d view, held to what ``_check_maps`` asks of a stack of maps."""
    if maps.dim() == 4 and maps.device.type == 'cuda' and maps.dtype == torch.float32 and maps.is_contiguous() and maps.shape[0] >= 1:
        sets = maps
    else:
        _check_maps(maps)
        sets = maps.unsqueeze(0)
    if sets.shape[1] < 1 or not (1 <= sets.shape[2] <= 128 and 1 <= sets.shape[3] <= 128):
        raise ValueError(f'region scores take maps of at least one row and 1..128 cells a side, got {tuple(maps.shape)}')
    return sets


def region_scores(maps: Optional[torch.Tensor], masks: torch.Tensor, map_hw: Optional[Tuple[int, int]] = None):
    """``daam_region_scores``: how much of every row's expanded heat map lies inside every mask.  ``maps=None`` with ``map_hw=(h, w)``:
    the footprints alone (``region_footprint``), scores ``None``.  ``maps`` is [rows, h, w] or
    [G, rows, h, w] fp32 on the device, ``masks`` [M, H, W] (or [H, W]) uint8 / bool (a byte != 0 is set; other dtypes through
    ``!= 0``; CPU masks are moved to the device).  Returns ``(scores, area, footprint)``: ``scores[..., m, t]`` = the sum over the set
    pixels of mask ``m`` of ``expand_word_map(maps[..., t], H, W, absolute=True)`` as fp32 [M, rows] (or [G, M, rows]), ``area``
    int32 [M] the exact pixel counts, ``footprint`` fp32 [M, h, w] the masks pulled back onto the maps' grid, which
    ``region_dots`` scores further map sets against.  No plane of H x W is written; more than 32 masks run in chunks of 32."""
    from .evaluate import _as_masks
    if maps is None:
        return region_footprint(masks, *map_hw) if map_hw is not None else _no_map_hw()
    sets = _check_map_sets(maps)
    masks = _as_masks(masks, 'masks', maps.device)
    if masks.device != maps.device:
        raise RuntimeError('daam_amd: maps and masks are on different devices')
    out = _region_chunks(masks, sets.shape[2], sets.shape[3], sets)
    scores, area, footprint = out[0] if len(out) == 1 else (torch.cat([o[0] for o in out], dim=1), torch.cat([o[1] for o in out]),
                                                           torch.cat([o[2] for o in out]))
    return (scores if maps.dim() == 4 else scores[0]), area, footprint


def _descriptors_on(device, arr) -> torch.Tensor:
    """A ctypes array of ``DaamKeyPlanes`` as a uint8 tensor on ``device``."""
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device, copy=True)


def map_gram(maps: torch.Tensor) -> torch.Tensor:
    """``daam_token_gram`` on one set of maps as a single f32 key: ``maps`` [rows, h, w] fp32 on the device (1..96 rows, 1..128 cells a
    side) -> fp32 ``[rows, rows]``, ``out[i][j] = sum_p maps[i][p] * maps[j][p]`` (``GlobalHeatMap.coattention``)."""
    _check_maps(maps)
    rows, h, w = maps.shape
    if not (1 <= rows <= 96 and 1 <= h <= 128 and 1 <= w <= 128):
        raise ValueError(f'a Gram matrix takes 1..96 rows of 1..128 cells a side, got {tuple(maps.shape)}')
    lib = nat.load_analysis()
    with torch.cuda.device(maps.device):
        desc = _descriptors_on(maps.device, (nat.KeyPlanes * 1)(nat.KeyPlanes(base=maps.data_ptr(), win_stride=0, h=h, w=w, n_win=1, pad=0)))
        scratch = torch.empty(lib.daam_token_gram_scratch_bytes(1, rows, h * w), dtype=torch.uint8, device=maps.device)
        gram = torch.empty(1, rows, rows, dtype=torch.float32, device=maps.device)
        nat.check_analysis(lib.daam_token_gram(desc.data_ptr(), 1, nat.DAAM_F32, rows, gram.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                               torch.cuda.current_stream(maps.device).cuda_stream))
    return gram[0]


def _no_map_hw():
    raise ValueError('region_scores(None, masks) needs map_hw=(h, w): the grid the footprints are pulled back onto')


def region_footprint(masks: torch.Tensor, h: int, w: int, device=None):
    """``region_scores`` without maps (``daam_region_scores`` with ``maps == NULL``): ``(None, area, footprint)`` of ``masks`` on an
    ``h x w`` grid, for ``region_dots`` / ``HeatMapEngine.key_scores``.  CPU masks are moved to ``device`` (default: the current one)."""
    from .evaluate import _as_masks
    h, w = int(h), int(w)
    if not (1 <= h <= 128 and 1 <= w <= 128):
        raise ValueError(f'region footprints take a grid of 1..128 cells a side, got {h} x {w}')
    masks = _as_masks(masks, 'masks', device)
    out = _region_chunks(masks, h, w, None)
    return (None, *(out[0][1:] if len(out) == 1 else (torch.cat([o[1] for o in out]), torch.cat([o[2] for o in out]))))


def _region_chunks(masks: torch.Tensor, h: int, w: int, sets: Optional[torch.Tensor]) -> list:
    """``daam_region_scores`` per 32 masks: ``[(scores or None, area, footprint)]``; ``sets`` [G, rows, h, w] or None (footprints only)."""
    n_sets, rows = (0, 0) if sets is None else sets.shape[:2]
    big_h, big_w = masks.shape[1:]
    lib = nat.load()
    out = []
    with torch.cuda.device(masks.device):
        stream = torch.cuda.current_stream(masks.device).cuda_stream
        for at in range(0, masks.shape[0], MAX_REGION_MASKS):
            chunk = masks[at:at + MAX_REGION_MASKS]
            n = chunk.shape[0]
            size = lib.daam_region_scores_workspace(n, big_h, big_w, h, w)
            if size == 0:
                raise ValueError(f'region scores: masks of {big_h} x {big_w} are outside the limits (H * W < 2^31)')
            ws = torch.empty(size, dtype=torch.uint8, device=masks.device)
            scores = None if sets is None else torch.empty(n_sets, n, rows, dtype=torch.float32, device=masks.device)
            area = torch.empty(n, dtype=torch.int32, device=masks.device)
            footprint = torch.empty(n, h, w, dtype=torch.float32, device=masks.device)
            nat.check(lib.daam_region_scores(chunk.data_ptr(), n, big_h, big_w, None if sets is None else sets.data_ptr(), n_sets, rows, h, w,
                                             footprint.data_ptr(), None if sets is None else scores.data_ptr(), area.data_ptr(),
                                             ws.data_ptr(), stream))
            out.append((scores, area, footprint))
    return out


def region_dots(maps: torch.Tensor, footprint: torch.Tensor) -> torch.Tensor:
    """``daam_region_dots``: the scores of a further map set ([rows, h, w] or [G, rows, h, w]) against the ``footprint`` [M, h, w]
    that ``region_scores`` returned -- bit for bit what ``region_scores`` gives for these maps and the masks behind the footprint."""
    sets = _check_map_sets(maps)
    if footprint.device != maps.device or footprint.dtype != torch.float32 or footprint.dim() != 3 or not footprint.is_contiguous():
        raise RuntimeError('daam_amd: footprint must be a contiguous fp32 [M, h, w] tensor on the maps\' device')
    if footprint.shape[1:] != sets.shape[2:]:
        raise ValueError(f'footprint of {tuple(footprint.shape[1:])} against maps of {tuple(sets.shape[2:])}')
    n_sets, rows, h, w = sets.shape
    out = []
    with torch.cuda.device(maps.device):
        for at in range(0, footprint.shape[0], MAX_REGION_MASKS):
            chunk = footprint[at:at + MAX_REGION_MASKS]
            scores = torch.empty(n_sets, chunk.shape[0], rows, dtype=torch.float32, device=maps.device)
            nat.check(nat.load().daam_region_dots(chunk.data_ptr(), chunk.shape[0], sets.data_ptr(), n_sets, rows, h, w, scores.data_ptr(),
                                                  torch.cuda.current_stream(maps.device).cuda_stream))
            out.append(scores)
    scores = out[0] if len(out) == 1 else torch.cat(out, dim=1)
    return scores if maps.dim() == 4 else scores[0]
