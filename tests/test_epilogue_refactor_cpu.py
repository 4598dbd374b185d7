"""The epilogue's shared device text (daam_amd/csrc/daam_epilogue.h) moved no machine code: every kernel of the
library has the fingerprint recorded for the parent commit (profiles/epilogue_refactor.json), the ten batched epilogue kernels
those their own pull requests recorded, and the helpers the header was made for are defined once in the source tree."""
import glob
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'daam_amd', 'csrc')
# the kernels of daam_word_masks.hip, daam_mask_matrix.hip and daam_region_scores.hip, by the profile that recorded them
NEWER = {'word_masks.json': ('word_masks_mean_kernel', 'word_masks_minmax_kernel', 'word_masks_out_kernel'),
         'mask_overlap_matrix.json': ('mask_matrix_zero_kernel', 'mask_matrix_kernelILb0', 'mask_matrix_kernelILb1'),
         'region_scores.json': ('region_tables_kernel', 'region_footprint_kernel', 'region_combine_kernel', 'region_dot_kernel')}


def _profile(name):
    return json.load(open(os.path.join(ROOT, 'profiles', name)))


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    lib = build.build(verbose=False)
    return lib, build.kernel_shas(lib)


def test_newer_epilogue_kernels_keep_their_recorded_fingerprints(built):
    _, have = built
    pinned = {}
    for profile, names in NEWER.items():
        rec = _profile(profile)['kernel_shas']
        for name in names:
            keys = [k for k in rec if name in k]
            assert len(keys) == 1, (profile, name)
            pinned[keys[0]] = rec[keys[0]]
    assert len(pinned) == 10
    assert {k: have.get(k) for k in pinned} == pinned


def test_every_kernel_has_the_parent_builds_fingerprint(built):
    _, have = built
    rec = _profile('epilogue_refactor.json')
    assert rec['kernel_shas_equal'] is True and rec['kernel_count'] == {'parent': 191, 'new': 191}
    assert rec['kernel_shas'] == rec['parent_kernel_shas'] and len(rec['kernel_shas']) == 191
    assert {k: have.get(k) for k in rec['kernel_shas']} == rec['kernel_shas']
    assert len(have) == 191


def test_existing_pins_still_hold(built):
    from test_tap_walk_cpu import PAIR_SHAS, WALK_SHAS
    _, have = built
    rec = _profile('r06_counters.json')['kernel_shas']
    assert len(rec) == 132
    assert {k: have.get(k) for k in rec} == rec
    assert {k: have.get(k) for k in PAIR_SHAS} == PAIR_SHAS
    assert {k: have.get(k) for k in WALK_SHAS} == WALK_SHAS


def _count(pattern, paths):
    """{file name: occurrences of the literal text} over the files that hold it"""
    out = {}
    for p in paths:
        n = open(p, errors='replace').read().count(pattern)
        if n:
            out[os.path.basename(p)] = n
    return out


def test_shared_helpers_are_defined_once():
    csrc = sorted(glob.glob(os.path.join(CSRC, '*')))
    tools = sorted(glob.glob(os.path.join(ROOT, 'tools', '*')))
    tools = [p for p in tools if os.path.isfile(p)]
    # Keys' weights: the Horner bodies start from `A = -0.75f`.  One device copy; the host's bicubic_table (daam_api.hip) builds the
    # finalize tables with its own and stays; tools/ holds none.
    assert _count('-0.75f', csrc) == {'daam_epilogue.h': 1, 'daam_api.hip': 1}
    assert _count('-0.75f', tools) == {}
    # the ordered encoding: `i ^ 0x7fffffff` once in enc_ordered and once in dec_ordered
    assert _count('i ^ 0x7fffffff', csrc) == {'daam_epilogue.h': 2}
    # the bit-set trio: mask_nonzero's constant (twice in its one expression), the second dot-product weight (twice in mask_bits16),
    # the byte-by-byte edge loop
    assert _count('0x7f7f7f7fu', csrc) == {'daam_epilogue.h': 2}
    assert _count('0x80402010u', csrc) == {'daam_epilogue.h': 2}
    assert _count('bits |= 1u << b', csrc) == {'daam_epilogue.h': 1}
    text = ''.join(open(p, errors='replace').read() for p in csrc)
    for name in ('cubic_coeffs', 'cubic_taps', 'cubic_row', 'enc_ordered', 'dec_ordered', 'store_for_host', 'mask_nonzero', 'mask_bits16',
                 'mask_bits16_edge'):
        assert len(re.findall(r'__device__ __forceinline__ \w+ \w*%s\(' % name, text)) == 1, name


def test_build_lists_and_exports(built):
    import subprocess
    from daam_amd import _native, build
    lib, _ = built
    assert 'daam_epilogue.hip' in build.SOURCES and 'daam_epilogue.h' in build.HEADERS
    assert all(os.path.exists(os.path.join(CSRC, f)) for f in build.SOURCES + build.HEADERS)
    nm = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    exported = sorted(re.findall(r' T (daam_\w+)$', nm, flags=re.M))
    assert exported == _profile('epilogue_refactor.json')['exported_symbols']
    assert _native.load().daam_abi_version() == 6
