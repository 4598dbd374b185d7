"""ctypes binding of ``libdaam_hip.so`` (C ABI: ``include/daam_hip.h``) and of the side libraries beside it.

There is no CPU or PyTorch fallback: if the HIP library is missing or no MI355X is visible
the import / first call fails loudly.  Build the library with ``python -m daam_amd.build``
(or ``__graft_entry__.build()``).

Each library is one ``Library`` record: its file, ABI version and a signature table ``{symbol: (argtypes, restype)}``.  The table is
the only list of symbols there is -- ``*_EXPORTS`` (what ``_open`` and the tests check) are its keys -- so a symbol cannot be checked
and not typed, or typed and not checked.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
from ctypes import POINTER, Structure, byref, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint8, c_void_p

DAAM_F16, DAAM_F32, DAAM_BF16 = 0, 1, 2
E_INVALID, E_STATE, E_NOMAPS, E_UNSUPPORTED = -1, -2, -3, -4


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


class KeyPlanes(Structure):
    """``DaamKeyPlanes`` (include/daam_analysis.h), 32 bytes."""
    _fields_ = [('base', c_void_p), ('win_stride', c_int64), ('h', c_int32), ('w', c_int32), ('n_win', c_int32), ('pad', c_int32)]


class RopeJob(Structure):
    """``daam_rope_job`` (include/daam_rope.h), 104 bytes."""
    _fields_ = [('x', c_void_p), ('out', c_void_p), ('cos', c_void_p), ('sin', c_void_p),
                ('batch', c_int32), ('heads', c_int32), ('rows', c_int32),
                ('x_stride_b', c_int64), ('x_stride_r', c_int64), ('x_stride_h', c_int64),
                ('out_stride_b', c_int64), ('out_stride_r', c_int64), ('out_stride_h', c_int64), ('table_stride', c_int64)]


@dataclasses.dataclass(frozen=True)
class Library:
    """How one library of the project is found, checked and typed."""
    file: str                       # basename; the library is built beside this module
    env: str                        # environment variable that names another file (read once, at import)
    what: str                       # what has no fallback, for the "missing" message
    abi_version: int
    version_fn: str
    error_fn: str
    table: dict                     # {symbol: (argtypes or None for an untyped symbol, restype)}
    path: str = dataclasses.field(init=False)

    def __post_init__(self):
        object.__setattr__(self, 'path', os.environ.get(self.env) or os.path.join(os.path.dirname(os.path.abspath(__file__)), self.file))

    @property
    def exports(self) -> tuple:
        return tuple(self.table)


def _sig(argtypes, restype=c_int):
    return argtypes, restype


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


def _bind(rec: Library, load_name: str):
    """``(load, check)`` of a library, to be bound to the module names ``load_name`` and its ``check_*``.  ``load()`` opens the file
    once, gives every symbol the types of the table and keeps the handle: after that it is one cell lookup and a return.  ``check(rc)``
    is one comparison when ``rc`` is 0; otherwise it asks whatever the module calls ``load_name`` at that moment (a stand-in a test
    installed included) for the error text."""
    handle = None

    def load() -> ctypes.CDLL:
        nonlocal handle
        if handle is not None:
            return handle
        lib = _open(rec.path, rec.what, rec.exports, rec.version_fn, rec.abi_version)
        for name, (argtypes, restype) in rec.table.items():
            fn = getattr(lib, name)
            if argtypes is not None:
                fn.argtypes = argtypes
            fn.restype = restype
        handle = lib
        return lib

    def check(rc: int) -> None:
        if rc != 0:
            msg = getattr(globals()[load_name](), rec.error_fn)()
            raise DaamError(rc, msg.decode() if msg else '')

    load.__name__ = load.__qualname__ = load_name
    check.__name__ = check.__qualname__ = 'check' + load_name[len('load'):]
    load.__doc__ = f'``{rec.file}`` ({rec.what}), opened, checked and typed on the first call; it has no fallback.'
    return load, check


# ---- libdaam_hip.so (C ABI: include/daam_hip.h): every symbol the header declares (tests check the library exports exactly these) ----
MAIN = Library('libdaam_hip.so', 'DAAM_HIP_LIB', 'the MI355X heat-map path', 6, 'daam_abi_version', 'daam_last_error', {
    'daam_abi_version': _sig(None),
    'daam_last_error': _sig(None, c_char_p),
    'daam_ctx_create': _sig([c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    'daam_ctx_destroy': _sig([c_void_p]),
    'daam_layer_configure': _sig([c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'daam_layer_acc': _sig([c_void_p, c_int, POINTER(c_void_p), POINTER(c_size_t)]),
    'daam_layer_touch': _sig([c_void_p, c_int, c_void_p]),
    'daam_layer_release': _sig([c_void_p, c_int]),
    'daam_ctx_set_time_bins': _sig([c_void_p, c_int, POINTER(c_int32)]),
    'daam_tap_steps': _sig([c_void_p, c_int, POINTER(c_int)]),
    'daam_reset': _sig([c_void_p, c_void_p]),
    'daam_tap_qk': _sig([c_void_p, c_int, c_void_p, c_void_p, POINTER(QKDesc), c_void_p]),
    'daam_tap_qk_enqueue': _sig([c_void_p, c_int, c_void_p, c_void_p, POINTER(QKDesc)]),
    'daam_tap_qk_enqueue_many': _sig([c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'daam_tap_pending': _sig([c_void_p, POINTER(c_int), POINTER(c_int)]),
    'daam_tap_flush': _sig([c_void_p, c_void_p]),
    'daam_tap_probs': _sig([c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    'daam_attend_supported': _sig([POINTER(AttendDesc), c_void_p, c_void_p, c_void_p, c_void_p]),
    'daam_attend': _sig([c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(AttendDesc), c_int, c_void_p]),
    'daam_key_offset': _sig([c_void_p, c_int, POINTER(c_int), POINTER(c_int)]),
    'daam_finalize': _sig([c_void_p, POINTER(c_uint8), c_int, c_void_p, c_void_p]),
    'daam_finalize_prepare': _sig([c_void_p, POINTER(c_uint8), c_int, c_void_p, c_void_p]),
    'daam_finalize_groups': _sig([c_void_p, POINTER(c_int32), c_int, POINTER(c_int32), c_void_p, c_size_t, c_void_p]),
    'daam_finalize_bins': _sig([c_void_p, POINTER(c_int32), c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32),
                                POINTER(c_int32), c_void_p, c_size_t, c_void_p]),
    'daam_epilogue_normalize': _sig([c_void_p, c_int, c_int, c_void_p]),
    'daam_word_heat_map': _sig([c_void_p, c_int, POINTER(c_int32), c_int, c_void_p, c_void_p, c_int, c_int,
                                c_int, c_float, c_void_p, c_void_p]),
    'daam_mask_overlap': _sig([c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    'daam_last_launch': _sig([c_void_p, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    'daam_last_flush': _sig([c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(ctypes.c_longlong)]),
    'daam_last_kernels': _sig([c_void_p, c_int, ctypes.c_char_p, c_int]),
    'daam_profile_enable': _sig([c_void_p, c_int]),
    'daam_profile_last_ms': _sig([c_void_p, c_int, POINTER(c_float)]),
    'daam_profile_history': _sig([c_void_p, c_int, POINTER(c_float), c_int, POINTER(c_int)]),
    'daam_clock_monitor_start': _sig([c_void_p, c_int, c_int]),
    'daam_clock_monitor_read': _sig([c_void_p, POINTER(c_float), c_int, POINTER(c_int)]),
    'daam_ctx_create_rect': _sig([c_int, c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    'daam_layer_configure_rect': _sig([c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'daam_epilogue_normalize_rect': _sig([c_void_p, c_int, c_int, c_int, c_void_p]),
    'daam_word_heat_map_rect': _sig([c_void_p, c_int, c_int, POINTER(c_int32), c_int, c_void_p, c_void_p, c_int, c_int,
                                     c_int, c_float, c_void_p, c_void_p]),
    'daam_word_masks': _sig([c_void_p, c_int, c_int, c_int, POINTER(c_int32), POINTER(c_int32), c_int, c_void_p, c_int, c_int,
                             c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    'daam_mask_overlap_matrix': _sig([c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'daam_region_scores_workspace': _sig([c_int, c_int, c_int, c_int, c_int], c_size_t),
    'daam_region_scores': _sig([c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    'daam_region_dots': _sig([c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
})

# ---- libdaam_analysis.so (C ABI: include/daam_analysis.h): key scores, token Gram matrices, heat maps of weighted key sets -----------
ANALYSIS = Library('libdaam_analysis.so', 'DAAM_ANALYSIS_LIB', 'per-key analysis', 3, 'daam_analysis_abi_version', 'daam_analysis_last_error', {
    'daam_key_scores': _sig([c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'daam_token_gram': _sig([c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'daam_token_gram_scratch_bytes': _sig([c_int, c_int, c_int], c_size_t),
    'daam_key_blend': _sig([c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int64, c_void_p, c_size_t,
                            c_void_p]),
    'daam_key_blend_scratch_bytes': _sig([c_int, c_int, c_int, c_int, c_int], c_size_t),
    'daam_analysis_abi_version': _sig(None),
    'daam_analysis_last_error': _sig(None, c_char_p),
})

# ---- libdaam_eval.so (C ABI: include/daam_eval.h): segmentation evaluation, the threshold sweeps --------------------------------------
EVAL = Library('libdaam_eval.so', 'DAAM_EVAL_LIB', 'the threshold sweep', 1, 'daam_eval_abi_version', 'daam_eval_last_error', {
    'daam_threshold_sweep': _sig([c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_void_p, c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'daam_threshold_sweep_workspace': _sig([c_int, c_int, c_int, c_int, c_int], c_size_t),
    'daam_eval_abi_version': _sig(None),
    'daam_eval_last_error': _sig(None, c_char_p),
})

# ---- libdaam_locate.so (C ABI: include/daam_locate.h): boxes, peaks, pointing hits ----------------------------------------------------
LOCATE = Library('libdaam_locate.so', 'DAAM_LOCATE_LIB', 'localize', 1, 'daam_locate_abi_version', 'daam_locate_last_error', {
    'daam_localize': _sig([c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_void_p, c_int,
                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    'daam_localize_workspace': _sig([c_int, c_int, c_int, c_int, c_int], c_size_t),
    'daam_locate_abi_version': _sig(None),
    'daam_locate_last_error': _sig(None, c_char_p),
})

# ---- libdaam_components.so (C ABI: include/daam_components.h): labels, areas, largest-blob boxes --------------------------------------
COMPONENTS = Library('libdaam_components.so', 'DAAM_COMPONENTS_LIB', 'mask_components', 1, 'daam_components_abi_version',
                     'daam_components_last_error', {
    'daam_mask_components': _sig([c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_size_t, c_void_p]),
    'daam_mask_components_workspace': _sig([c_int, c_int, c_int, c_int], c_size_t),
    'daam_components_abi_version': _sig(None),
    'daam_components_last_error': _sig(None, c_char_p),
})

# ---- libdaam_refine.so (C ABI: include/daam_refine.h): local-affinity propagation of soft word maps along the image -------------------
REFINE = Library('libdaam_refine.so', 'DAAM_REFINE_LIB', 'refine', 1, 'daam_refine_abi_version', 'daam_refine_last_error', {
    'daam_refine_affinity': _sig([c_void_p, c_int, c_int, c_int, POINTER(c_int32), c_int, c_float, c_void_p, c_void_p]),
    'daam_refine_apply': _sig([c_void_p, POINTER(c_int32), c_int, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_size_t, c_void_p]),
    'daam_refine_weights_bytes': _sig([c_int, c_int, c_int], c_size_t),
    'daam_refine_workspace': _sig([c_int, c_int, c_int], c_size_t),
    'daam_refine_abi_version': _sig(None),
    'daam_refine_last_error': _sig(None, c_char_p),
})

# ---- libdaam_selfaff.so (C ABI: include/daam_self_affinity.h): head-summed softmax(Q K^T) of attn1, word maps propagated along it ----
SELFAFF = Library('libdaam_selfaff.so', 'DAAM_SELFAFF_LIB', 'self_affinity', 1, 'daam_self_affinity_abi_version',
                  'daam_self_affinity_last_error', {
    'daam_self_affinity_accumulate': _sig([c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int64, c_int64, c_int64, c_int64,
                                           c_int64, c_int64, c_float, c_float, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'daam_self_affinity_propagate': _sig([c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    'daam_self_affinity_workspace': _sig([c_int, c_int, c_int], c_size_t),
    'daam_self_affinity_propagate_workspace': _sig([c_int, c_int], c_size_t),
    'daam_self_affinity_abi_version': _sig(None),
    'daam_self_affinity_last_error': _sig(None, c_char_p),
})

LIBRARIES = (MAIN, ANALYSIS, EVAL, LOCATE, COMPONENTS, REFINE, SELFAFF)

# ---- libdaam_joint.so (C ABI: include/daam_joint_tap.h): the text columns of the joint softmax of an MMDiT attention call -------------
# A record beside LIBRARIES, not in it: `build.build()` does not make this file (`build.build_joint` does).
JOINT_LIBRARY = Library('libdaam_joint.so', 'DAAM_JOINT_LIB', 'trace_joint', 1, 'daam_joint_tap_abi_version', 'daam_joint_tap_last_error', {
    'daam_joint_tap_accumulate': _sig([c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                       c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                                       c_float, c_float, c_int, c_void_p, c_int64, c_void_p, c_size_t, c_void_p]),
    'daam_joint_tap_workspace': _sig([c_int, c_int, c_int], c_size_t),
    'daam_joint_tap_abi_version': _sig(None),
    'daam_joint_tap_last_error': _sig(None, c_char_p),
})

# ---- libdaam_rope.so (C ABI: include/daam_rope.h): the rotary embedding of a FLUX-class attention call, up to four tensors a launch ----
# Beside LIBRARIES like JOINT_LIBRARY: `build.build_rope` makes the file.
ROPE_LIBRARY = Library('libdaam_rope.so', 'DAAM_ROPE_LIB', 'trace_flux', 1, 'daam_rope_abi_version', 'daam_rope_last_error', {
    'daam_rope_apply': _sig([POINTER(RopeJob), c_int, c_int, c_int, c_void_p]),
    'daam_rope_abi_version': _sig(None),
    'daam_rope_last_error': _sig(None, c_char_p),
})

# ---- libdaam_jointaff.so (C ABI: include/daam_joint_affinity.h): the image columns of the joint softmax, from the tap's statistics ----
# Beside LIBRARIES like JOINT_LIBRARY: `build.build_joint_affinity` makes the file.
JOINT_AFFINITY_LIBRARY = Library('libdaam_jointaff.so', 'DAAM_JOINT_AFFINITY_LIB', 'self_affinity on trace_joint / trace_flux', 1,
                                 'daam_joint_affinity_abi_version', 'daam_joint_affinity_last_error', {
    'daam_joint_affinity_accumulate': _sig([c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_int, c_int,
                                            c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_float, c_float, c_int, c_void_p,
                                            c_void_p]),
    'daam_joint_affinity_stats_bytes': _sig([c_int, c_int, c_int], c_size_t),
    'daam_joint_affinity_abi_version': _sig(None),
    'daam_joint_affinity_last_error': _sig(None, c_char_p),
})

# ---- libdaam_discover.so (C ABI: include/daam_discover.h): segments from a self-affinity -- prepare, pair_kl, merge, labels -----------
# Beside LIBRARIES like JOINT_LIBRARY: `build.build_discover` makes the file.
DISCOVER_LIBRARY = Library('libdaam_discover.so', 'DAAM_DISCOVER_LIB', 'SelfAffinity.discover', 1, 'daam_discover_abi_version',
                           'daam_discover_last_error', {
    'daam_discover_prepare': _sig([c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'daam_discover_pair_kl': _sig([c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'daam_discover_merge': _sig([c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    'daam_discover_labels': _sig([c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'daam_discover_abi_version': _sig(None),
    'daam_discover_last_error': _sig(None, c_char_p),
})

# ---- libdaam_jointattend.so (C ABI: include/daam_joint_attend.h): the joint attention itself, statistics as a by-product -------------
# Beside LIBRARIES like JOINT_LIBRARY: `build.build_joint_attend` makes the file.
JOINT_ATTEND_LIBRARY = Library('libdaam_jointattend.so', 'DAAM_JOINT_ATTEND_LIB', 'trace_joint(attend=True)', 1,
                               'daam_joint_attend_abi_version', 'daam_joint_attend_last_error', {
    'daam_joint_attend_forward': _sig([c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                       c_int, c_int, c_int, c_int, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), c_float,
                                       c_void_p, c_size_t, c_void_p]),
    'daam_joint_attend_text': _sig([c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_int, c_int, c_int, c_int64, c_int64,
                                    c_int64, c_int64, c_int64, c_int64, c_float, c_float, c_int, c_void_p, c_int64, c_void_p]),
    'daam_joint_attend_stats_bytes': _sig([c_int, c_int, c_int], c_size_t),
    'daam_joint_attend_abi_version': _sig(None),
    'daam_joint_attend_last_error': _sig(None, c_char_p),
})

# The names the engine, the tools and the tests use: one line per library, all of it read off the record.
LIB_NAME, LIB_PATH, ABI_VERSION, EXPORTS = MAIN.file, MAIN.path, MAIN.abi_version, MAIN.exports
ANALYSIS_LIB_NAME, ANALYSIS_LIB_PATH, ANALYSIS_ABI_VERSION, ANALYSIS_EXPORTS = ANALYSIS.file, ANALYSIS.path, ANALYSIS.abi_version, ANALYSIS.exports
EVAL_LIB_NAME, EVAL_LIB_PATH, EVAL_ABI_VERSION, EVAL_EXPORTS = EVAL.file, EVAL.path, EVAL.abi_version, EVAL.exports
LOCATE_LIB_NAME, LOCATE_LIB_PATH, LOCATE_ABI_VERSION, LOCATE_EXPORTS = LOCATE.file, LOCATE.path, LOCATE.abi_version, LOCATE.exports
COMPONENTS_LIB_NAME, COMPONENTS_LIB_PATH, COMPONENTS_ABI_VERSION, COMPONENTS_EXPORTS = \
    COMPONENTS.file, COMPONENTS.path, COMPONENTS.abi_version, COMPONENTS.exports
REFINE_LIB_NAME, REFINE_LIB_PATH, REFINE_ABI_VERSION, REFINE_EXPORTS = REFINE.file, REFINE.path, REFINE.abi_version, REFINE.exports
SELFAFF_LIB_NAME, SELFAFF_LIB_PATH, SELFAFF_ABI_VERSION, SELFAFF_EXPORTS = SELFAFF.file, SELFAFF.path, SELFAFF.abi_version, SELFAFF.exports
load, check = _bind(MAIN, 'load')
load_analysis, check_analysis = _bind(ANALYSIS, 'load_analysis')
load_eval, check_eval = _bind(EVAL, 'load_eval')
load_locate, check_locate = _bind(LOCATE, 'load_locate')
load_components, check_components = _bind(COMPONENTS, 'load_components')
load_refine, check_refine = _bind(REFINE, 'load_refine')
load_self_affinity, check_self_affinity = _bind(SELFAFF, 'load_self_affinity')
JOINT_LIB_NAME, JOINT_LIB_PATH, JOINT_ABI_VERSION, JOINT_EXPORTS = JOINT_LIBRARY.file, JOINT_LIBRARY.path, JOINT_LIBRARY.abi_version, JOINT_LIBRARY.exports
load_joint, check_joint = _bind(JOINT_LIBRARY, 'load_joint')
ROPE_LIB_NAME, ROPE_LIB_PATH, ROPE_ABI_VERSION, ROPE_EXPORTS = ROPE_LIBRARY.file, ROPE_LIBRARY.path, ROPE_LIBRARY.abi_version, ROPE_LIBRARY.exports
load_rope, check_rope = _bind(ROPE_LIBRARY, 'load_rope')
JOINT_AFFINITY_LIB_NAME, JOINT_AFFINITY_LIB_PATH, JOINT_AFFINITY_ABI_VERSION, JOINT_AFFINITY_EXPORTS = \
    JOINT_AFFINITY_LIBRARY.file, JOINT_AFFINITY_LIBRARY.path, JOINT_AFFINITY_LIBRARY.abi_version, JOINT_AFFINITY_LIBRARY.exports
load_joint_affinity, check_joint_affinity = _bind(JOINT_AFFINITY_LIBRARY, 'load_joint_affinity')
DISCOVER_LIB_NAME, DISCOVER_LIB_PATH, DISCOVER_ABI_VERSION, DISCOVER_EXPORTS = \
    DISCOVER_LIBRARY.file, DISCOVER_LIBRARY.path, DISCOVER_LIBRARY.abi_version, DISCOVER_LIBRARY.exports
load_discover, check_discover = _bind(DISCOVER_LIBRARY, 'load_discover')
JOINT_ATTEND_LIB_NAME, JOINT_ATTEND_LIB_PATH, JOINT_ATTEND_ABI_VERSION, JOINT_ATTEND_EXPORTS = \
    JOINT_ATTEND_LIBRARY.file, JOINT_ATTEND_LIBRARY.path, JOINT_ATTEND_LIBRARY.abi_version, JOINT_ATTEND_LIBRARY.exports
load_joint_attend, check_joint_attend = _bind(JOINT_ATTEND_LIBRARY, 'load_joint_attend')

__all__ = ['load', 'check', 'DaamError', 'QKDesc', 'AttendDesc', 'DAAM_F16', 'DAAM_F32', 'DAAM_BF16', 'EXPORTS', 'LIB_PATH',
           'byref', 'c_void_p', 'c_int', 'c_uint8', 'c_int32', 'c_size_t', 'E_NOMAPS']
