"""ctypes binding of ``libdaam_hip.so`` (C ABI: ``include/daam_hip.h``).

There is no CPU or PyTorch fallback: if the HIP library is missing or no MI355X is visible
the import / first call fails loudly.  Build the library with ``python -m daam_amd.build``
(or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, byref, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint8, c_void_p

LIB_NAME = 'libdaam_hip.so'
LIB_PATH = os.environ.get('DAAM_HIP_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)

ABI_VERSION = 6
DAAM_F16, DAAM_F32, DAAM_BF16 = 0, 1, 2
E_INVALID, E_STATE, E_NOMAPS, E_UNSUPPORTED = -1, -2, -3, -4

# every symbol include/daam_hip.h declares (tests check the library exports exactly these)
EXPORTS = (
    'daam_abi_version', 'daam_last_error', 'daam_ctx_create', 'daam_ctx_destroy', 'daam_layer_configure',
    'daam_layer_acc', 'daam_layer_touch', 'daam_layer_release', 'daam_ctx_set_time_bins', 'daam_tap_steps', 'daam_reset', 'daam_tap_qk', 'daam_tap_qk_enqueue', 'daam_tap_qk_enqueue_many', 'daam_tap_pending', 'daam_tap_flush',
    'daam_tap_probs', 'daam_attend_supported', 'daam_attend', 'daam_key_offset', 'daam_finalize', 'daam_finalize_prepare', 'daam_finalize_groups', 'daam_finalize_bins', 'daam_epilogue_normalize', 'daam_word_heat_map', 'daam_mask_overlap',
    'daam_last_launch', 'daam_last_flush', 'daam_last_kernels', 'daam_profile_enable', 'daam_profile_last_ms', 'daam_profile_history', 'daam_clock_monitor_start', 'daam_clock_monitor_read',
    'daam_ctx_create_rect', 'daam_layer_configure_rect', 'daam_epilogue_normalize_rect', 'daam_word_heat_map_rect',
    'daam_word_masks', 'daam_mask_overlap_matrix', 'daam_region_scores_workspace', 'daam_region_scores', 'daam_region_dots',
)


class DaamError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f'libdaam_hip error {code}: {message}')
        self.code = code


class QKDesc(Structure):
    """``DaamQKDesc`` (include/daam_hip.h)."""
    _fields_ = [
        ('in_dtype', c_int32), ('batch', c_int32), ('heads', c_int32), ('hw', c_int32), ('tokens', c_int32),
        ('head_dim', c_int32), ('round_logits', c_int32), ('scale', c_float),
        ('q_stride_b', c_int64), ('q_stride_h', c_int64), ('q_stride_p', c_int64),
        ('k_stride_b', c_int64), ('k_stride_h', c_int64), ('k_stride_t', c_int64),
    ]


class AttendDesc(Structure):
    """``DaamAttendDesc`` (include/daam_hip.h)."""
    _fields_ = [
        ('qk', QKDesc),
        ('v_stride_b', c_int64), ('v_stride_h', c_int64), ('v_stride_t', c_int64),
        ('o_stride_b', c_int64), ('o_stride_h', c_int64), ('o_stride_p', c_int64),
    ]


_lib = None


def _open(path: str, what: str, exports, version_fn: str, version: int) -> ctypes.CDLL:
    """Open a library of the project: it exists, has every symbol of ``exports`` and reports ``version``, or RuntimeError (there is
    no fallback: missing or stale is an error that names the file and the remedy)."""
    if not os.path.exists(path):
        raise RuntimeError(f'{path} is missing: {what} has no fallback. '
                           f'Build it with `python -m daam_amd.build` (needs hipcc, --offload-arch=gfx950).')
    lib = ctypes.CDLL(path)
    # a library built before an entry point was added: same ABI version, fewer symbols -- as stale as a version mismatch
    missing = [name for name in exports if not hasattr(lib, name)]
    if missing:
        raise RuntimeError(f'{path}: lacks {", ".join(missing)} (stale build); rebuild')
    built = getattr(lib, version_fn)
    built.restype = c_int
    if built() != version:
        raise RuntimeError(f'{path}: ABI version {built()} != {version}; rebuild')
    return lib


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    lib = _open(LIB_PATH, 'the MI355X heat-map path', EXPORTS, 'daam_abi_version', ABI_VERSION)
    lib.daam_last_error.restype = c_char_p
    lib.daam_ctx_create.argtypes = [c_int, c_int, c_int, c_int, POINTER(c_void_p)]
    lib.daam_ctx_destroy.argtypes = [c_void_p]
    lib.daam_layer_configure.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p]
    lib.daam_layer_acc.argtypes = [c_void_p, c_int, POINTER(c_void_p), POINTER(c_size_t)]
    lib.daam_layer_touch.argtypes = [c_void_p, c_int, c_void_p]
    lib.daam_layer_release.argtypes = [c_void_p, c_int]
    lib.daam_reset.argtypes = [c_void_p, c_void_p]
    lib.daam_tap_qk.argtypes = [c_void_p, c_int, c_void_p, c_void_p, POINTER(QKDesc), c_void_p]
    lib.daam_tap_qk_enqueue.argtypes = [c_void_p, c_int, c_void_p, c_void_p, POINTER(QKDesc)]
    lib.daam_tap_qk_enqueue_many.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.daam_tap_pending.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int)]
    lib.daam_tap_flush.argtypes = [c_void_p, c_void_p]
    lib.daam_tap_probs.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]
    lib.daam_attend_supported.argtypes = [POINTER(AttendDesc), c_void_p, c_void_p, c_void_p, c_void_p]
    lib.daam_attend.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(AttendDesc), c_int, c_void_p]
    lib.daam_key_offset.argtypes = [c_void_p, c_int, POINTER(c_int), POINTER(c_int)]
    lib.daam_finalize.argtypes = [c_void_p, POINTER(c_uint8), c_int, c_void_p, c_void_p]
    lib.daam_finalize_prepare.argtypes = [c_void_p, POINTER(c_uint8), c_int, c_void_p, c_void_p]
    lib.daam_finalize_groups.argtypes = [c_void_p, POINTER(c_int32), c_int, POINTER(c_int32), c_void_p, c_size_t, c_void_p]
    lib.daam_finalize_bins.argtypes = [c_void_p, POINTER(c_int32), c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                       POINTER(c_int32), c_void_p, c_size_t, c_void_p]
    lib.daam_ctx_set_time_bins.argtypes = [c_void_p, c_int, POINTER(c_int32)]
    lib.daam_tap_steps.argtypes = [c_void_p, c_int, POINTER(c_int)]
    lib.daam_epilogue_normalize.argtypes = [c_void_p, c_int, c_int, c_void_p]
    lib.daam_word_heat_map.argtypes = [c_void_p, c_int, POINTER(c_int32), c_int, c_void_p, c_void_p, c_int, c_int,
                                       c_int, c_float, c_void_p, c_void_p]
    lib.daam_ctx_create_rect.argtypes = [c_int, c_int, c_int, c_int, c_int, POINTER(c_void_p)]
    lib.daam_layer_configure_rect.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]
    lib.daam_epilogue_normalize_rect.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p]
    lib.daam_word_heat_map_rect.argtypes = [c_void_p, c_int, c_int, POINTER(c_int32), c_int, c_void_p, c_void_p, c_int, c_int,
                                            c_int, c_float, c_void_p, c_void_p]
    lib.daam_word_masks.argtypes = [c_void_p, c_int, c_int, c_int, POINTER(c_int32), POINTER(c_int32), c_int, c_void_p, c_int, c_int,
                                    c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.daam_mask_overlap.argtypes =[c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.daam_mask_overlap_matrix.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.daam_region_scores_workspace.argtypes = [c_int, c_int, c_int, c_int, c_int]
    lib.daam_region_scores.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p]
    lib.daam_region_dots.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
    lib.daam_profile_history.argtypes = [c_void_p, c_int, POINTER(c_float), c_int, POINTER(c_int)]
    lib.daam_last_launch.argtypes = [c_void_p, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int)]
    lib.daam_last_flush.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(ctypes.c_longlong)]
    lib.daam_last_kernels.argtypes = [c_void_p, c_int, ctypes.c_char_p, c_int]
    lib.daam_profile_enable.argtypes = [c_void_p, c_int]
    lib.daam_profile_last_ms.argtypes = [c_void_p, c_int, POINTER(c_float)]
    lib.daam_clock_monitor_start.argtypes = [c_void_p, c_int, c_int]
    lib.daam_clock_monitor_read.argtypes = [c_void_p, POINTER(c_float), c_int, POINTER(c_int)]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ('daam_last_error', 'daam_region_scores_workspace'):
            fn.restype = c_int
    lib.daam_region_scores_workspace.restype = c_size_t
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().daam_last_error()
        raise DaamError(rc, msg.decode() if msg else '')


# ---- libdaam_analysis.so (C ABI: include/daam_analysis.h) -------------------------------------------------------------------------
ANALYSIS_LIB_NAME = 'libdaam_analysis.so'
ANALYSIS_LIB_PATH = os.environ.get('DAAM_ANALYSIS_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), ANALYSIS_LIB_NAME)
ANALYSIS_ABI_VERSION = 3
ANALYSIS_EXPORTS = ('daam_key_scores', 'daam_token_gram', 'daam_token_gram_scratch_bytes', 'daam_key_blend', 'daam_key_blend_scratch_bytes',
                    'daam_analysis_abi_version', 'daam_analysis_last_error')


class KeyPlanes(Structure):
    """``DaamKeyPlanes`` (include/daam_analysis.h), 32 bytes."""
    _fields_ = [('base', c_void_p), ('win_stride', c_int64), ('h', c_int32), ('w', c_int32), ('n_win', c_int32), ('pad', c_int32)]


_analysis = None


def load_analysis() -> ctypes.CDLL:
    """The per-key analysis library (key scores, token Gram matrices, heat maps of weighted key sets); like ``load`` it has no
    fallback."""
    global _analysis
    if _analysis is not None:
        return _analysis
    lib = _open(ANALYSIS_LIB_PATH, 'per-key analysis', ANALYSIS_EXPORTS, 'daam_analysis_abi_version', ANALYSIS_ABI_VERSION)
    lib.daam_key_scores.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]
    lib.daam_key_scores.restype = c_int
    lib.daam_token_gram.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.daam_token_gram.restype = c_int
    lib.daam_token_gram_scratch_bytes.argtypes = [c_int, c_int, c_int]
    lib.daam_token_gram_scratch_bytes.restype = c_size_t
    lib.daam_key_blend.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_size_t,
                                   c_void_p]
    lib.daam_key_blend.restype = c_int
    lib.daam_key_blend_scratch_bytes.argtypes = [c_int, c_int, c_int, c_int, c_int]
    lib.daam_key_blend_scratch_bytes.restype = c_size_t
    lib.daam_analysis_last_error.restype = c_char_p
    _analysis = lib
    return lib


def check_analysis(rc: int) -> None:
    if rc != 0:
        msg = load_analysis().daam_analysis_last_error()
        raise DaamError(rc, msg.decode() if msg else '')


# ---- libdaam_eval.so (C ABI: include/daam_eval.h) ---------------------------------------------------------------------------------
EVAL_LIB_NAME = 'libdaam_eval.so'
EVAL_LIB_PATH = os.environ.get('DAAM_EVAL_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), EVAL_LIB_NAME)
EVAL_ABI_VERSION = 1
EVAL_EXPORTS = ('daam_threshold_sweep', 'daam_threshold_sweep_workspace', 'daam_eval_abi_version', 'daam_eval_last_error')

_eval = None


def load_eval() -> ctypes.CDLL:
    """The segmentation-evaluation library (threshold sweeps); like ``load`` it has no fallback."""
    global _eval
    if _eval is not None:
        return _eval
    lib = _open(EVAL_LIB_PATH, 'the threshold sweep', EVAL_EXPORTS, 'daam_eval_abi_version', EVAL_ABI_VERSION)
    lib.daam_threshold_sweep.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_void_p, c_int,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.daam_threshold_sweep.restype = c_int
    lib.daam_threshold_sweep_workspace.argtypes = [c_int, c_int, c_int, c_int, c_int]
    lib.daam_threshold_sweep_workspace.restype = c_size_t
    lib.daam_eval_last_error.restype = c_char_p
    _eval = lib
    return lib


def check_eval(rc: int) -> None:
    if rc != 0:
        msg = load_eval().daam_eval_last_error()
        raise DaamError(rc, msg.decode() if msg else '')


# ---- libdaam_locate.so (C ABI: include/daam_locate.h) -----------------------------------------------------------------------------
LOCATE_LIB_NAME = 'libdaam_locate.so'
LOCATE_LIB_PATH = os.environ.get('DAAM_LOCATE_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), LOCATE_LIB_NAME)
LOCATE_ABI_VERSION = 1
LOCATE_EXPORTS = ('daam_localize', 'daam_localize_workspace', 'daam_locate_abi_version', 'daam_locate_last_error')

_locate = None


def load_locate() -> ctypes.CDLL:
    """The localisation library (boxes, peaks, pointing hits); like ``load`` it has no fallback."""
    global _locate
    if _locate is not None:
        return _locate
    lib = _open(LOCATE_LIB_PATH, 'localize', LOCATE_EXPORTS, 'daam_locate_abi_version', LOCATE_ABI_VERSION)
    lib.daam_localize.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_void_p, c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.daam_localize.restype = c_int
    lib.daam_localize_workspace.argtypes = [c_int, c_int, c_int, c_int, c_int]
    lib.daam_localize_workspace.restype = c_size_t
    lib.daam_locate_last_error.restype = c_char_p
    _locate = lib
    return lib


def check_locate(rc: int) -> None:
    if rc != 0:
        msg = load_locate().daam_locate_last_error()
        raise DaamError(rc, msg.decode() if msg else '')


# ---- libdaam_components.so (C ABI: include/daam_components.h) ---------------------------------------------------------------------
COMPONENTS_LIB_NAME = 'libdaam_components.so'
COMPONENTS_LIB_PATH = os.environ.get('DAAM_COMPONENTS_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), COMPONENTS_LIB_NAME)
COMPONENTS_ABI_VERSION = 1
COMPONENTS_EXPORTS = ('daam_mask_components', 'daam_mask_components_workspace', 'daam_components_abi_version', 'daam_components_last_error')

_components = None


def load_components() -> ctypes.CDLL:
    """The connected-components library (labels, areas, largest-blob boxes); like ``load`` it has no fallback."""
    global _components
    if _components is not None:
        return _components
    lib = _open(COMPONENTS_LIB_PATH, 'mask_components', COMPONENTS_EXPORTS, 'daam_components_abi_version', COMPONENTS_ABI_VERSION)
    lib.daam_mask_components.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_size_t, c_void_p]
    lib.daam_mask_components.restype = c_int
    lib.daam_mask_components_workspace.argtypes = [c_int, c_int, c_int, c_int]
    lib.daam_mask_components_workspace.restype = c_size_t
    lib.daam_components_last_error.restype = c_char_p
    _components = lib
    return lib


def check_components(rc: int) -> None:
    if rc != 0:
        msg = load_components().daam_components_last_error()
        raise DaamError(rc, msg.decode() if msg else '')


# ---- libdaam_refine.so (C ABI: include/daam_refine.h) ------------------------------------------------------------------------------
REFINE_LIB_NAME = 'libdaam_refine.so'
REFINE_LIB_PATH = os.environ.get('DAAM_REFINE_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), REFINE_LIB_NAME)
REFINE_ABI_VERSION = 1
REFINE_EXPORTS = ('daam_refine_affinity', 'daam_refine_apply', 'daam_refine_weights_bytes', 'daam_refine_workspace',
                  'daam_refine_abi_version', 'daam_refine_last_error')

_refine = None


def load_refine() -> ctypes.CDLL:
    """The refinement library (local-affinity propagation of soft word maps along the image); like ``load`` it has no fallback."""
    global _refine
    if _refine is not None:
        return _refine
    lib = _open(REFINE_LIB_PATH, 'refine', REFINE_EXPORTS, 'daam_refine_abi_version', REFINE_ABI_VERSION)
    lib.daam_refine_affinity.argtypes = [c_void_p, c_int, c_int, c_int, POINTER(c_int32), c_int, c_float, c_void_p, c_void_p]
    lib.daam_refine_affinity.restype = c_int
    lib.daam_refine_apply.argtypes = [c_void_p, POINTER(c_int32), c_int, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_size_t, c_void_p]
    lib.daam_refine_apply.restype = c_int
    lib.daam_refine_weights_bytes.argtypes = [c_int, c_int, c_int]
    lib.daam_refine_weights_bytes.restype = c_size_t
    lib.daam_refine_workspace.argtypes = [c_int, c_int, c_int]
    lib.daam_refine_workspace.restype = c_size_t
    lib.daam_refine_last_error.restype = c_char_p
    _refine = lib
    return lib


def check_refine(rc: int) -> None:
    if rc != 0:
        msg = load_refine().daam_refine_last_error()
        raise DaamError(rc, msg.decode() if msg else '')


# ---- libdaam_selfaff.so (C ABI: include/daam_self_affinity.h) ----------------------------------------------------------------------
SELFAFF_LIB_NAME = 'libdaam_selfaff.so'
SELFAFF_LIB_PATH = os.environ.get('DAAM_SELFAFF_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), SELFAFF_LIB_NAME)
SELFAFF_ABI_VERSION = 1
SELFAFF_EXPORTS = ('daam_self_affinity_accumulate', 'daam_self_affinity_propagate', 'daam_self_affinity_workspace',
                   'daam_self_affinity_propagate_workspace', 'daam_self_affinity_abi_version', 'daam_self_affinity_last_error')

_selfaff = None


def load_self_affinity() -> ctypes.CDLL:
    """The self-attention affinity library (head-summed softmax(Q K^T) of attn1, propagation of word maps along it); like ``load`` it
    has no fallback."""
    global _selfaff
    if _selfaff is not None:
        return _selfaff
    lib = _open(SELFAFF_LIB_PATH, 'self_affinity', SELFAFF_EXPORTS, 'daam_self_affinity_abi_version', SELFAFF_ABI_VERSION)
    lib.daam_self_affinity_accumulate.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64,
                                                  c_int64, c_int64, c_float, c_float, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.daam_self_affinity_accumulate.restype = c_int
    lib.daam_self_affinity_propagate.argtypes = [c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]
    lib.daam_self_affinity_propagate.restype = c_int
    lib.daam_self_affinity_workspace.argtypes = [c_int, c_int, c_int]
    lib.daam_self_affinity_workspace.restype = c_size_t
    lib.daam_self_affinity_propagate_workspace.argtypes = [c_int, c_int]
    lib.daam_self_affinity_propagate_workspace.restype = c_size_t
    lib.daam_self_affinity_last_error.restype = c_char_p
    _selfaff = lib
    return lib


def check_self_affinity(rc: int) -> None:
    if rc != 0:
        msg = load_self_affinity().daam_self_affinity_last_error()
        raise DaamError(rc, msg.decode() if msg else '')


__all__ = ['load', 'check', 'DaamError', 'QKDesc', 'AttendDesc', 'DAAM_F16', 'DAAM_F32', 'DAAM_BF16', 'EXPORTS', 'LIB_PATH',
           'byref', 'c_void_p', 'c_int', 'c_uint8', 'c_int32', 'c_size_t', 'E_NOMAPS']
