"""Build ``libdaam_hip.so`` in-tree with hipcc for gfx950:  ``python -m daam_amd.build``."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from functools import partial
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ['daam_api.hip', 'daam_tap_api.hip', 'daam_finalize_api.hip', 'daam_kernels.hip', 'daam_tap_mfma.hip', 'daam_tap_d64.hip', 'daam_tap_wide.hip', 'daam_tap_chunk.hip', 'daam_tap_slab.hip', 'daam_tap_pair.hip', 'daam_tap_walk.hip', 'daam_attend_d64.hip', 'daam_finalize.hip', 'daam_finalize_pipe.hip', 'daam_fin_bins.hip', 'daam_finalize_rect.hip', 'daam_epilogue.hip', 'daam_word_masks.hip', 'daam_mask_matrix.hip', 'daam_region_scores.hip']
HEADERS = ['daam_types.h', 'daam_elem.h', 'daam_finalize.h', 'daam_fin_bins.h', 'daam_fin_rect.h', 'daam_ctx.h', 'daam_tap_common.h', 'daam_tap16.h', 'daam_tap16_softmax.h', 'daam_tap_tile64.h', 'daam_tap_walk.h', 'daam_tap_rows.h', 'daam_epilogue.h', 'daam_tap_d64_body.inc', 'daam_finalize_pipe_asm_r16.inc', 'daam_finalize_pipe_asm_bf16.inc', 'daam_finalize_pipe_asm_f32.inc',
           'daam_finalize_pipe_prefill_r16.inc', 'daam_finalize_pipe_prefill_f32.inc', 'daam_fin_kernel_body.inc', 'daam_fin_up_kernel_body.inc', 'daam_fin_down2_kernel_body.inc', 'daam_fin_pipe_kernel_body.inc', 'daam_word_expand_body.inc', os.path.join('..', '..', 'include', 'daam_hip.h')]
OUT = os.path.join(HERE, 'libdaam_hip.so')
HIPCC_FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-fvisibility=hidden']    # one command: compile and link


class SideLibrary(NamedTuple):
    """A stateless library beside ``libdaam_hip.so``: ``sources`` go through one hipcc command into ``out``; ``headers`` are what else
    it is made of (files under csrc/, or relative to it), for ``side_stale``."""
    name: str
    sources: list
    headers: list
    out: str


def _api(header: str) -> str:
    return os.path.join('..', '..', 'include', header)


# The MFMA row-softmax parts and host checks that the self-affinity and the joint tap share: read by those two alone.
ROWSOFTMAX = 'daam_rowsoftmax32.h'

# Every side library is kept out of SOURCES / HEADERS so that csrc_sha() and the kernels of libdaam_hip.so stay what the committed
# profiles were measured on.  The order is the build order.
SIDE_LIBRARIES = (
    # libdaam_analysis.so (include/daam_analysis.h): the three per-key analyses (key scores, token Gram, weighted key maps), with no
    # context.  Its sources read the first library's headers.
    SideLibrary('analysis', ['daam_key_scores.hip', 'daam_token_gram.hip', 'daam_key_blend.hip'],
                ['daam_key_planes.h', 'daam_key_scores.h', 'daam_token_gram.h', 'daam_key_blend.h', 'daam_finalize.h', 'daam_epilogue.h',
                 'daam_elem.h', 'daam_types.h', _api('daam_hip.h'), _api('daam_analysis.h')], os.path.join(HERE, 'libdaam_analysis.so')),
    # libdaam_eval.so (include/daam_eval.h): segmentation evaluation -- the threshold sweep.  It restates what it shares with
    # daam_word_masks.hip and reads daam_epilogue.h.
    SideLibrary('eval', ['daam_threshold_sweep.hip'], ['daam_epilogue.h', 'daam_types.h', _api('daam_hip.h'), _api('daam_eval.h')],
                os.path.join(HERE, 'libdaam_eval.so')),
    # libdaam_locate.so (include/daam_locate.h): localisation -- boxes, peaks and pointing hits.  Like the evaluation library it
    # restates what it shares with daam_word_masks.hip through daam_epilogue.h.
    SideLibrary('locate', ['daam_locate.hip'], ['daam_epilogue.h', 'daam_types.h', _api('daam_hip.h'), _api('daam_locate.h')],
                os.path.join(HERE, 'libdaam_locate.so')),
    # libdaam_components.so (include/daam_components.h): connected components of byte masks.  It reads daam_epilogue.h for the
    # bit-set helpers alone.
    SideLibrary('components', ['daam_components.hip'], ['daam_epilogue.h', 'daam_types.h', _api('daam_hip.h'), _api('daam_components.h')],
                os.path.join(HERE, 'libdaam_components.so')),
    # libdaam_refine.so (include/daam_refine.h): image-guided refinement of soft word maps (local-affinity propagation).  It reads no
    # header of csrc/.
    SideLibrary('refine', ['daam_refine.hip'], [_api('daam_hip.h'), _api('daam_refine.h')], os.path.join(HERE, 'libdaam_refine.so')),
    # libdaam_selfaff.so (include/daam_self_affinity.h): the self-attention affinity (head-summed softmax(Q K^T) of attn1, an MFMA
    # kernel of its own) and the propagation of word maps along it.  Of csrc/ it reads ROWSOFTMAX alone.
    SideLibrary('selfaff', ['daam_self_affinity.hip'], [ROWSOFTMAX, _api('daam_hip.h'), _api('daam_self_affinity.h')],
                os.path.join(HERE, 'libdaam_selfaff.so')),
)
ANALYSIS, EVAL, LOCATE, COMPONENTS, REFINE, SELFAFF = SIDE_LIBRARIES


def csrc_sha() -> str:
    """Fingerprint of the kernel sources (csrc/*.hip, *.h and the C header): ties committed profiler summaries
    (profiles/*.json) to the build they were measured on."""
    import hashlib
    h = hashlib.sha256()
    for f in sorted(SOURCES + HEADERS):
        with open(os.path.join(HERE, 'csrc', f), 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()[:12]


def kernel_shas(lib: str = OUT) -> dict:
    """``{mangled kernel name: fingerprint of its machine code}`` for every kernel in a built library: the gfx950 code objects
    are cut out of the offload bundles in ``.hip_fatbin`` and the bytes of every function symbol hashed.  Unlike ``csrc_sha``
    this does not change when a source file gains an ``#if``-guarded experiment or when another kernel file is added, and it
    does change when the compiler emits different code for an untouched source: it is what ties a committed profiler summary to
    the kernels of THIS build (bench.py ``load_counters``)."""
    import hashlib
    import struct
    data = open(lib, 'rb').read()
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    out = {}
    pos = data.find(magic)
    while pos >= 0:
        n, = struct.unpack_from('<Q', data, pos + len(magic))
        o = pos + len(magic) + 8
        for _ in range(n):
            off, size, ts = struct.unpack_from('<QQQ', data, o)
            o += 24
            triple = data[o:o + ts].decode()
            o += ts
            if 'gfx950' in triple and size:
                out.update(_elf_function_shas(data[pos + off:pos + off + size], hashlib))
        pos = data.find(magic, pos + 1)
    return out


def _elf_function_shas(elf: bytes, hashlib) -> dict:
    import struct
    if elf[:4] != b'\x7fELF' or elf[4] != 2:
        return {}
    shoff, = struct.unpack_from('<Q', elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from('<HHH', elf, 0x3A)
    secs = [struct.unpack_from('<IIQQQQIIQQ', elf, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for (_, typ, _, _, off, size, link, _, _, entsize) in secs:
        if typ != 2:                                         # SHT_SYMTAB
            continue
        str_off = secs[link][4]
        for i in range(size // entsize):
            name_i, info, _, shndx, value, fsize = struct.unpack_from('<IBBHQQ', elf, off + i * entsize)
            if (info & 0xF) != 2 or not fsize or shndx >= len(secs):      # STT_FUNC with a body
                continue
            end = elf.index(b'\0', str_off + name_i)
            name = elf[str_off + name_i:end].decode()
            sec = secs[shndx]
            start = sec[4] + (value - sec[3])
            out[name] = hashlib.sha256(elf[start:start + fsize]).hexdigest()[:12]
    return out


def hipcc() -> str:
    exe = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(exe):
        raise RuntimeError('hipcc not found (need ROCm with gfx950 support)')
    return exe


def stale() -> bool:
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    deps = [os.path.join(HERE, 'csrc', f) for f in SOURCES + HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def side_stale(lib: SideLibrary) -> bool:
    if not os.path.exists(lib.out):
        return True
    t = os.path.getmtime(lib.out)
    return any(os.path.getmtime(os.path.join(HERE, 'csrc', f)) > t for f in lib.sources + lib.headers)


def build_side(lib: SideLibrary, force: bool = False, verbose: bool = True) -> str:
    """A side library: one hipcc command, when it is missing or older than what it is made of."""
    if not force and not side_stale(lib):
        return lib.out
    cmd = [hipcc(), *HIPCC_FLAGS, *[os.path.join(HERE, 'csrc', f) for f in lib.sources], '-o', lib.out]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return lib.out


# The names tests, tools and the entry point use, all of them read off the records.
ANALYSIS_SOURCES, ANALYSIS_HEADERS, ANALYSIS_OUT = ANALYSIS[1:]
EVAL_SOURCES, EVAL_HEADERS, EVAL_LIB = EVAL[1:]
LOCATE_SOURCES, LOCATE_HEADERS, LOCATE_LIB = LOCATE[1:]
COMPONENTS_SOURCES, COMPONENTS_HEADERS, COMPONENTS_LIB = COMPONENTS[1:]
REFINE_SOURCES, REFINE_HEADERS, REFINE_LIB = REFINE[1:]
SELFAFF_SOURCES, SELFAFF_HEADERS, SELFAFF_LIB = SELFAFF[1:]
analysis_stale, eval_stale, locate_stale, components_stale, refine_stale, self_affinity_stale = (partial(side_stale, lib) for lib in SIDE_LIBRARIES)
build_analysis, build_eval, build_locate, build_components, build_refine, build_self_affinity = (partial(build_side, lib) for lib in SIDE_LIBRARIES)


# libdaam_joint.so (include/daam_joint_tap.h): the joint-attention tap of MMDiT pipelines (text columns of a softmax over text and image
# keys, MFMA kernels of its own).  Of csrc/ it reads ROWSOFTMAX alone.  The record stands beside SIDE_LIBRARIES, not in it: build() makes
# the six of the tuple, `python -m daam_amd.build` and the entry point make this one after them, by the same recipe.
JOINT = SideLibrary('joint', ['daam_joint_tap.hip'], [ROWSOFTMAX, _api('daam_hip.h'), _api('daam_joint_tap.h')],
                    os.path.join(HERE, 'libdaam_joint.so'))
JOINT_SOURCES, JOINT_HEADERS, JOINT_LIB = JOINT[1:]
joint_stale, build_joint = partial(side_stale, JOINT), partial(build_side, JOINT)

# libdaam_rope.so (include/daam_rope.h): the rotary embedding of a FLUX-class attention call on up to four tensors in one launch, what
# trace_flux runs before the joint tap.  It reads no header of csrc/.  Like JOINT it stands beside SIDE_LIBRARIES and is made after it.
ROPE = SideLibrary('rope', ['daam_rope.hip'], [_api('daam_hip.h'), _api('daam_rope.h')], os.path.join(HERE, 'libdaam_rope.so'))
ROPE_SOURCES, ROPE_HEADERS, ROPE_LIB = ROPE[1:]
rope_stale, build_rope = partial(side_stale, ROPE), partial(build_side, ROPE)

# libdaam_jointaff.so (include/daam_joint_affinity.h): the image columns of the joint softmax, summed into an affinity matrix from the
# statistics the joint tap has just written (`trace_joint` / `trace_flux` with self_affinity=True).  It reads no header of csrc/: the
# readers of ROWSOFTMAX stay the two above, and this library restates the few device helpers it shares with them.
# Like JOINT and ROPE it stands beside SIDE_LIBRARIES and is made after them.
JOINT_AFFINITY = SideLibrary('jointaff', ['daam_joint_affinity.hip'], [_api('daam_hip.h'), _api('daam_joint_affinity.h')],
                             os.path.join(HERE, 'libdaam_jointaff.so'))
JOINT_AFFINITY_SOURCES, JOINT_AFFINITY_HEADERS, JOINT_AFFINITY_LIB = JOINT_AFFINITY[1:]
joint_affinity_stale, build_joint_affinity = partial(side_stale, JOINT_AFFINITY), partial(build_side, JOINT_AFFINITY)

# libdaam_discover.so (include/daam_discover.h): segments from a self-affinity without a word list -- probability rows and their
# logarithms, the symmetric KL divergence of anchor rows against all rows (a tiled VALU kernel), the merge of member rows and the label
# map of the resized proposals (`SelfAffinity.discover`).  It reads no header of csrc/.  Like JOINT, ROPE and
# JOINT_AFFINITY it stands beside SIDE_LIBRARIES and is made after them.
DISCOVER = SideLibrary('discover', ['daam_discover.hip'], [_api('daam_hip.h'), _api('daam_discover.h')],
                       os.path.join(HERE, 'libdaam_discover.so'))
DISCOVER_SOURCES, DISCOVER_HEADERS, DISCOVER_LIB = DISCOVER[1:]
discover_stale, build_discover = partial(side_stale, DISCOVER), partial(build_side, DISCOVER)

# libdaam_jointattend.so (include/daam_joint_attend.h): the joint attention of an MMDiT block itself -- softmax(Q K^T) V for image and
# text queries with the image rows' statistics as a by-product of the key walk -- and the text columns from those statistics
# (`trace_joint(attend=True)`).  It reads no header of csrc/ and restates the device helpers it shares with the joint tap,
# as JOINT_AFFINITY does.  Like JOINT, ROPE, JOINT_AFFINITY and DISCOVER it stands beside SIDE_LIBRARIES and is made after them.
JOINT_ATTEND = SideLibrary('jointattend', ['daam_joint_attend.hip'], [_api('daam_hip.h'), _api('daam_joint_attend.h')],
                           os.path.join(HERE, 'libdaam_jointattend.so'))
JOINT_ATTEND_SOURCES, JOINT_ATTEND_HEADERS, JOINT_ATTEND_LIB = JOINT_ATTEND[1:]
joint_attend_stale, build_joint_attend = partial(side_stale, JOINT_ATTEND), partial(build_side, JOINT_ATTEND)


def fastpath_out() -> str:
    import sysconfig
    return os.path.join(HERE, '_fastpath' + sysconfig.get_config_var('EXT_SUFFIX'))


def build_fastpath(force: bool = False, verbose: bool = True) -> str:
    """``daam_amd._fastpath``: the host-side tap recorder (csrc/daam_fastpath.cpp), a CPython extension
    compiled against the torch headers of the running interpreter (host code only, no device code)."""
    import sysconfig
    import torch
    from torch.utils import cpp_extension as ext
    src = os.path.join(HERE, 'csrc', 'daam_fastpath.cpp')
    out = fastpath_out()
    if not force and os.path.exists(out) and os.path.getmtime(out) >= os.path.getmtime(src):
        return out
    lib_dirs = ext.library_paths()
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    # host code only; the HIP platform define and headers are for c10::hip::getCurrentHIPStream (the recorder launches
    # daam_attend on torch's current stream), nothing here is compiled for the device
    cmd = ['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-D__HIP_PLATFORM_AMD__', '-DUSE_ROCM',
           f'-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}',
           '-I' + sysconfig.get_paths()['include'], *['-I' + p for p in ext.include_paths()], '-I' + os.path.join(rocm, 'include'),
           src, '-o', out, *['-L' + p for p in lib_dirs], *['-Wl,-rpath,' + p for p in lib_dirs],
           '-ltorch_python', '-ltorch', '-ltorch_cpu', '-lc10', '-lc10_hip']
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return out


def build_variant(out: str, flags, verbose: bool = True) -> str:
    """A/B builds for kernel experiments (tools/): the same sources with extra ``-D`` flags into another file; load it with
    ``DAAM_HIP_LIB=<out>``."""
    cmd = [hipcc(), *HIPCC_FLAGS, *flags, *[os.path.join(HERE, 'csrc', f) for f in SOURCES], '-o', out]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return out


def _deps_of(src: str) -> list:
    """Headers / generated includes a source depends on (every HEADERS entry: they are few and cheap to stat)."""
    return [os.path.join(HERE, 'csrc', src)] + [os.path.join(HERE, 'csrc', h) for h in HEADERS]


def build(force: bool = False, verbose: bool = True, jobs: int = 0) -> str:
    """One object per source (``daam_amd/build/*.o``, compiled in parallel, only when the source or a header is newer), one link.
    The device code of a source is the same whether it is compiled alone or in one hipcc command with the others (no -fgpu-rdc):
    ``kernel_shas()`` of the library is what ties profiles to a build."""
    from concurrent.futures import ThreadPoolExecutor
    build_fastpath(force, verbose)
    for lib in SIDE_LIBRARIES:
        build_side(lib, force, verbose)
    if not force and not stale():
        return OUT
    objdir = os.path.join(HERE, 'build')
    os.makedirs(objdir, exist_ok=True)
    flags = [f for f in HIPCC_FLAGS if f != '-shared']
    todo = []
    for f in SOURCES:
        obj = os.path.join(objdir, f + '.o')
        if force or not os.path.exists(obj) or any(os.path.getmtime(d) > os.path.getmtime(obj) for d in _deps_of(f)):
            todo.append([hipcc(), *flags, '-c', os.path.join(HERE, 'csrc', f), '-o', obj])

    def run(cmd):
        if verbose:
            print(' '.join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    with ThreadPoolExecutor(max_workers=jobs or min(6, os.cpu_count() or 1)) as ex:
        list(ex.map(run, todo))
    # the link: no -O3 / -std=, and -shared ahead of -fPIC as this command has always had them
    run([hipcc(), *[HIPCC_FLAGS[i] for i in (0, 4, 3, 5)], *[os.path.join(objdir, f + '.o') for f in SOURCES], '-o', OUT])
    return OUT


if __name__ == '__main__':
    build(force='--force' in sys.argv)
    build_joint(force='--force' in sys.argv)
    build_rope(force='--force' in sys.argv)
    build_joint_affinity(force='--force' in sys.argv)
    build_joint_attend(force='--force' in sys.argv)
    build_discover(force='--force' in sys.argv)
    print(OUT)
