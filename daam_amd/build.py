"""Build ``libdaam_hip.so`` in-tree with hipcc for gfx950:  ``python -m daam_amd.build``."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ['daam_api.hip', 'daam_tap_api.hip', 'daam_finalize_api.hip', 'daam_kernels.hip', 'daam_tap_mfma.hip', 'daam_tap_d64.hip', 'daam_tap_wide.hip', 'daam_tap_chunk.hip', 'daam_tap_slab.hip', 'daam_tap_pair.hip', 'daam_tap_walk.hip', 'daam_attend_d64.hip', 'daam_finalize.hip', 'daam_finalize_pipe.hip', 'daam_fin_bins.hip', 'daam_finalize_rect.hip', 'daam_epilogue.hip', 'daam_word_masks.hip', 'daam_mask_matrix.hip', 'daam_region_scores.hip']
HEADERS = ['daam_types.h', 'daam_elem.h', 'daam_finalize.h', 'daam_fin_bins.h', 'daam_fin_rect.h', 'daam_ctx.h', 'daam_tap_common.h', 'daam_tap16.h', 'daam_tap16_softmax.h', 'daam_tap_tile64.h', 'daam_tap_walk.h', 'daam_tap_rows.h', 'daam_epilogue.h', 'daam_tap_d64_body.inc', 'daam_finalize_pipe_asm_r16.inc', 'daam_finalize_pipe_asm_bf16.inc', 'daam_finalize_pipe_asm_f32.inc',
           'daam_finalize_pipe_prefill_r16.inc', 'daam_finalize_pipe_prefill_f32.inc', 'daam_fin_kernel_body.inc', 'daam_fin_up_kernel_body.inc', 'daam_fin_down2_kernel_body.inc', 'daam_fin_pipe_kernel_body.inc', 'daam_word_expand_body.inc', os.path.join('..', '..', 'include', 'daam_hip.h')]
OUT = os.path.join(HERE, 'libdaam_hip.so')
# libdaam_analysis.so (include/daam_analysis.h): the one side library, the three per-key analyses (key scores, token Gram, weighted
# key maps), with no context.  It is kept out of SOURCES / HEADERS so that csrc_sha() and the kernels of libdaam_hip.so stay what the
# committed profiles were measured on.  Its sources read the first library's headers.
ANALYSIS_SOURCES = ['daam_key_scores.hip', 'daam_token_gram.hip', 'daam_key_blend.hip']
ANALYSIS_HEADERS = ['daam_key_planes.h', 'daam_key_scores.h', 'daam_token_gram.h', 'daam_key_blend.h', 'daam_finalize.h', 'daam_epilogue.h',
                    'daam_elem.h', 'daam_types.h', os.path.join('..', '..', 'include', 'daam_hip.h'),
                    os.path.join('..', '..', 'include', 'daam_analysis.h')]
ANALYSIS_OUT = os.path.join(HERE, 'libdaam_analysis.so')
# libdaam_eval.so (include/daam_eval.h): segmentation evaluation -- the threshold sweep.  It restates what it shares with
# daam_word_masks.hip and reads daam_epilogue.h; like the analysis library it stays out of SOURCES / HEADERS.
EVAL_SOURCES = ['daam_threshold_sweep.hip']
EVAL_HEADERS = ['daam_epilogue.h', 'daam_types.h', os.path.join('..', '..', 'include', 'daam_hip.h'), os.path.join('..', '..', 'include', 'daam_eval.h')]
EVAL_LIB = os.path.join(HERE, 'libdaam_eval.so')
# libdaam_locate.so (include/daam_locate.h): localisation -- boxes, peaks and pointing hits.  Like the evaluation library it restates
# what it shares with daam_word_masks.hip through daam_epilogue.h and stays out of every list above.
LOCATE_SOURCES = ['daam_locate.hip']
LOCATE_HEADERS = ['daam_epilogue.h', 'daam_types.h', os.path.join('..', '..', 'include', 'daam_hip.h'), os.path.join('..', '..', 'include', 'daam_locate.h')]
LOCATE_LIB = os.path.join(HERE, 'libdaam_locate.so')
# libdaam_components.so (include/daam_components.h): connected components of byte masks.  It reads daam_epilogue.h for the bit-set
# helpers alone and stays out of every list above.
COMPONENTS_SOURCES = ['daam_components.hip']
COMPONENTS_HEADERS = ['daam_epilogue.h', 'daam_types.h', os.path.join('..', '..', 'include', 'daam_hip.h'),
                      os.path.join('..', '..', 'include', 'daam_components.h')]
COMPONENTS_LIB = os.path.join(HERE, 'libdaam_components.so')
# libdaam_refine.so (include/daam_refine.h): image-guided refinement of soft word maps (local-affinity propagation).  It reads no
# header of csrc/ and stays out of every list above.
REFINE_SOURCES = ['daam_refine.hip']
REFINE_HEADERS = [os.path.join('..', '..', 'include', 'daam_hip.h'), os.path.join('..', '..', 'include', 'daam_refine.h')]
REFINE_LIB = os.path.join(HERE, 'libdaam_refine.so')
# libdaam_selfaff.so (include/daam_self_affinity.h): the self-attention affinity (head-summed softmax(Q K^T) of attn1, an MFMA kernel
# of its own) and the propagation of word maps along it.  It reads no header of csrc/ and stays out of every list above.
SELFAFF_SOURCES = ['daam_self_affinity.hip']
SELFAFF_HEADERS = [os.path.join('..', '..', 'include', 'daam_hip.h'), os.path.join('..', '..', 'include', 'daam_self_affinity.h')]
SELFAFF_LIB = os.path.join(HERE, 'libdaam_selfaff.so')


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


def analysis_stale() -> bool:
    if not os.path.exists(ANALYSIS_OUT):
        return True
    t = os.path.getmtime(ANALYSIS_OUT)
    return any(os.path.getmtime(os.path.join(HERE, 'csrc', f)) > t for f in ANALYSIS_SOURCES + ANALYSIS_HEADERS)


def build_analysis(force: bool = False, verbose: bool = True) -> str:
    """``libdaam_analysis.so``: one hipcc command, when it is missing or older than what it is made of."""
    if not force and not analysis_stale():
        return ANALYSIS_OUT
    cmd = [hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-fvisibility=hidden',
           *[os.path.join(HERE, 'csrc', f) for f in ANALYSIS_SOURCES], '-o', ANALYSIS_OUT]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return ANALYSIS_OUT


def eval_stale() -> bool:
    if not os.path.exists(EVAL_LIB):
        return True
    t = os.path.getmtime(EVAL_LIB)
    return any(os.path.getmtime(os.path.join(HERE, 'csrc', f)) > t for f in EVAL_SOURCES + EVAL_HEADERS)


def build_eval(force: bool = False, verbose: bool = True) -> str:
    """``libdaam_eval.so``: one hipcc command, when it is missing or older than what it is made of."""
    if not force and not eval_stale():
        return EVAL_LIB
    cmd = [hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-fvisibility=hidden',
           *[os.path.join(HERE, 'csrc', f) for f in EVAL_SOURCES], '-o', EVAL_LIB]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return EVAL_LIB


def locate_stale() -> bool:
    if not os.path.exists(LOCATE_LIB):
        return True
    t = os.path.getmtime(LOCATE_LIB)
    return any(os.path.getmtime(os.path.join(HERE, 'csrc', f)) > t for f in LOCATE_SOURCES + LOCATE_HEADERS)


def build_locate(force: bool = False, verbose: bool = True) -> str:
    """``libdaam_locate.so``: one hipcc command, when it is missing or older than what it is made of."""
    if not force and not locate_stale():
        return LOCATE_LIB
    cmd = [hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-fvisibility=hidden',
           *[os.path.join(HERE, 'csrc', f) for f in LOCATE_SOURCES], '-o', LOCATE_LIB]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return LOCATE_LIB


def components_stale() -> bool:
    if not os.path.exists(COMPONENTS_LIB):
        return True
    t = os.path.getmtime(COMPONENTS_LIB)
    return any(os.path.getmtime(os.path.join(HERE, 'csrc', f)) > t for f in COMPONENTS_SOURCES + COMPONENTS_HEADERS)


def build_components(force: bool = False, verbose: bool = True) -> str:
    """``libdaam_components.so``: one hipcc command, when it is missing or older than what it is made of."""
    if not force and not components_stale():
        return COMPONENTS_LIB
    cmd = [hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-fvisibility=hidden',
           *[os.path.join(HERE, 'csrc', f) for f in COMPONENTS_SOURCES], '-o', COMPONENTS_LIB]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return COMPONENTS_LIB


def refine_stale() -> bool:
    if not os.path.exists(REFINE_LIB):
        return True
    t = os.path.getmtime(REFINE_LIB)
    return any(os.path.getmtime(os.path.join(HERE, 'csrc', f)) > t for f in REFINE_SOURCES + REFINE_HEADERS)


def build_refine(force: bool = False, verbose: bool = True) -> str:
    """``libdaam_refine.so``: one hipcc command, when it is missing or older than what it is made of."""
    if not force and not refine_stale():
        return REFINE_LIB
    cmd = [hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-fvisibility=hidden',
           *[os.path.join(HERE, 'csrc', f) for f in REFINE_SOURCES], '-o', REFINE_LIB]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return REFINE_LIB


def self_affinity_stale() -> bool:
    if not os.path.exists(SELFAFF_LIB):
        return True
    t = os.path.getmtime(SELFAFF_LIB)
    return any(os.path.getmtime(os.path.join(HERE, 'csrc', f)) > t for f in SELFAFF_SOURCES + SELFAFF_HEADERS)


def build_self_affinity(force: bool = False, verbose: bool = True) -> str:
    """``libdaam_selfaff.so``: one hipcc command, when it is missing or older than what it is made of."""
    if not force and not self_affinity_stale():
        return SELFAFF_LIB
    cmd = [hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-fvisibility=hidden',
           *[os.path.join(HERE, 'csrc', f) for f in SELFAFF_SOURCES], '-o', SELFAFF_LIB]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return SELFAFF_LIB


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
    cmd = [hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-fvisibility=hidden', *flags,
           *[os.path.join(HERE, 'csrc', f) for f in SOURCES], '-o', out]
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
    build_analysis(force, verbose)
    build_eval(force, verbose)
    build_locate(force, verbose)
    build_components(force, verbose)
    build_refine(force, verbose)
    build_self_affinity(force, verbose)
    if not force and not stale():
        return OUT
    objdir = os.path.join(HERE, 'build')
    os.makedirs(objdir, exist_ok=True)
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden']
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
    run([hipcc(), '--offload-arch=gfx950', '-shared', '-fPIC', '-fvisibility=hidden',
         *[os.path.join(objdir, f + '.o') for f in SOURCES], '-o', OUT])
    return OUT


if __name__ == '__main__':
    build(force='--force' in sys.argv)
    print(OUT)
