"""``libdaam_analysis.so`` without a GPU, said once for its three analyses (key scores, token Gram, key blend): it is the one side
library, built by one hipcc command beside ``libdaam_hip.so``; it exports what its header declares; every kernel of both libraries
is the machine code its committed profile was measured on; no kernel instance has scratch.  That a deleted library is rebuilt alone
is said for every side library in ``test_side_libraries_cpu.py``; what each call does with its arguments is in ``test_key_scores_cpu.py``, ``test_token_gram_cpu.py`` and ``test_key_blend_cpu.py``."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import _libcheck as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build(verbose=False)
    return build.ANALYSIS_OUT


def _profile_shas(name):
    return json.load(open(os.path.join(ROOT, 'profiles', name)))['kernel_shas']


def test_one_side_library_builds_and_exports_its_header(built):
    from daam_amd import _native as nat, build
    assert os.path.exists(built) and os.path.exists(build.OUT) and not build.stale() and not build.analysis_stale()
    assert build.ANALYSIS_SOURCES == ['daam_key_scores.hip', 'daam_token_gram.hip', 'daam_key_blend.hip']
    assert not any('analysis' in os.path.basename(f) for f in build.HEADERS)
    exported = LC.exported(built)
    assert exported == LC.declared('daam_analysis.h') == sorted(nat.ANALYSIS_EXPORTS) and len(exported) == 7
    assert {'daam_key_scores', 'daam_token_gram', 'daam_token_gram_scratch_bytes', 'daam_key_blend', 'daam_key_blend_scratch_bytes'} <= set(exported)
    assert nat.load_analysis().daam_analysis_abi_version() == 3 == nat.ANALYSIS_ABI_VERSION
    assert ctypes.sizeof(nat.KeyPlanes) == 32
    # no further library: the build knows two outputs (what it writes: test_side_libraries_cpu.py, test_deleted_library_is_rebuilt_alone),
    # and neither the build nor the binding has a name of the library the blend once had to itself
    assert sorted(n for n in vars(build) if n.endswith('OUT')) == ['ANALYSIS_OUT', 'OUT']
    assert not [n for mod in (build, nat) for n in vars(mod) if 'blend' in n.lower()]


def test_analysis_header_is_c99(tmp_path):
    """The public header compiles as C99 under -pedantic, as daam_hip.h is held to (test_host_logic.py)."""
    src = tmp_path / 'use.c'
    src.write_text('#include "daam_analysis.h"\nint main(void) { return sizeof(DaamKeyPlanes) == 32 && DAAM_ANALYSIS_ABI_VERSION == 3 ? 0 : 1; }\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'use')],
                   check=True)
    assert subprocess.run([str(tmp_path / 'use')]).returncode == 0


def test_the_blend_source_defines_nothing_the_library_shares():
    from daam_amd import build
    src = open(os.path.join(build.HERE, 'csrc', 'daam_key_blend.hip')).read() + open(os.path.join(build.HERE, 'csrc', 'daam_key_blend.h')).read()
    for name in ('key_planes_ok', 'cubic_taps', 'cubic_row', 'cubic_coeffs', 'fin_dispatch', 'fin_launch', 'key_args_check', r'\w+_fail'):
        assert not re.search(r'\b(?:float|int|bool|void|hipError_t)\s+%s\(' % name, src), name
    assert 'struct KeyElem' not in src and 'typedef' not in src and 'thread_local' not in src
    assert 'atomic' not in src.lower().replace('no floating-point atomic', '')


def test_every_kernel_is_what_it_was(built):
    from daam_amd import _native as nat, build
    rec = _profile_shas('finalize_launch_refactor.json')
    have = build.kernel_shas(build.OUT)
    assert len(have) == 191 and {k: have.get(k) for k in rec} == rec
    assert nat.load().daam_abi_version() == 6
    # the side library: each kernel the machine code its analysis was profiled on.  key_scores_kernel on f16, bf16, f32; the token
    # Gram's 16-bit path (2 dtypes x 3 row-block counts), f32 path (3 dtypes x 3) and join; key_blend_kernel on the three and its join
    parts = [_profile_shas(name) for name in ('key_scores.json', 'token_gram.json', 'key_blend.json')]
    assert [len(p) for p in parts] == [3, 16, 4] and len(set().union(*parts)) == 23
    want = {k: v for p in parts for k, v in p.items()}
    mine = build.kernel_shas(built)
    assert len(mine) == 23 and mine == want
    count = lambda word: sum(word in k for k in mine)
    assert [count(w) for w in ('key_scores_kernel', 'token_gram_kernel', 'token_gram_join_kernel', 'key_blend_kernel', 'key_blend_join_kernel')] \
        == [3, 15, 1, 3, 1]


def test_no_instance_has_scratch(built):
    """A resource check only: private segment size 0 and the private-segment enable bit clear in every kernel descriptor."""
    from daam_amd import build
    names = list(build.kernel_shas(built))
    assert len(names) == 23
    LC.assert_no_scratch(built, names)
