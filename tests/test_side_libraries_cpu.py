"""The side libraries (``build.SIDE_LIBRARIES``, ``_native.LIBRARIES``) without a GPU, said once for all six: each is
built by the one recipe beside ``libdaam_hip.so`` out of files no other library lists; it exports what its header declares and what
its binding table types; the header is C99; no kernel has scratch; a deleted library is rebuilt alone.  Then the two things that
hold the table-driven build and binding to what the hand-written ones did: the argv of every hipcc command, and the types every
symbol carries after loading.  What each library computes is in its own file.

Adding a library: one ``SideLibrary`` in ``daam_amd/build.py``, one ``Library`` in ``daam_amd/_native.py``, one row of ``EXPECT``."""
import os
import subprocess
import types

import pytest

import _libcheck as LC
from daam_amd import _native as nat, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What each library is held to, as the per-library tests stated it before they were gathered here (pinned values, not read off the
# code under test).  ``names``: the prefix of its module-level names in build / _native and the suffix of its functions;
# ``fragments``: what no other library's lists may mention; ``own``: headers under csrc/ that are this library's alone.
EXPECT = {
    'analysis': dict(header='daam_analysis.h', basename='libdaam_analysis.so', exports=7, abi=3, kernels=23, argtypes={},
                     names=('ANALYSIS', 'analysis', 'OUT'), env='DAAM_ANALYSIS_LIB', macro='DAAM_ANALYSIS_ABI_VERSION', fn='daam_key_scores',
                     own=('daam_key_scores.h', 'daam_token_gram.h', 'daam_key_blend.h', 'daam_key_planes.h'),
                     fragments=('analysis', 'key_scores', 'token_gram', 'key_blend', 'key_planes')),
    'eval': dict(header='daam_eval.h', basename='libdaam_eval.so', exports=4, abi=1, kernels=4, argtypes={'daam_threshold_sweep': 17},
                 names=('EVAL', 'eval', 'LIB'), env='DAAM_EVAL_LIB', macro='DAAM_EVAL_ABI_VERSION', fn='daam_threshold_sweep', own=(),
                 fragments=('daam_eval', 'threshold_sweep')),
    'locate': dict(header='daam_locate.h', basename='libdaam_locate.so', exports=4, abi=1, kernels=4, argtypes={'daam_localize': 19},
                   names=('LOCATE', 'locate', 'LIB'), env='DAAM_LOCATE_LIB', macro='DAAM_LOCATE_ABI_VERSION', fn='daam_localize', own=(),
                   fragments=('locate',)),
    'components': dict(header='daam_components.h', basename='libdaam_components.so', exports=4, abi=1, kernels=7,
                       argtypes={'daam_mask_components': 16}, names=('COMPONENTS', 'components', 'LIB'), env='DAAM_COMPONENTS_LIB',
                       macro='DAAM_COMPONENTS_ABI_VERSION', fn='daam_mask_components', own=(), fragments=('components',)),
    'refine': dict(header='daam_refine.h', basename='libdaam_refine.so', exports=6, abi=1, kernels=13,
                   argtypes={'daam_refine_affinity': 9, 'daam_refine_apply': 15}, names=('REFINE', 'refine', 'LIB'), env='DAAM_REFINE_LIB',
                   macro='DAAM_REFINE_ABI_VERSION', fn='daam_refine_apply', own=(), fragments=('refine',)),
    'selfaff': dict(header='daam_self_affinity.h', basename='libdaam_selfaff.so', exports=6, abi=1, kernels=29,
                    argtypes={'daam_self_affinity_accumulate': 20, 'daam_self_affinity_propagate': 9},
                    names=('SELFAFF', 'self_affinity', 'LIB'), env='DAAM_SELFAFF_LIB', macro='DAAM_SELF_AFFINITY_ABI_VERSION',
                    fn='daam_self_affinity_accumulate', own=(), fragments=('self_affinity', 'selfaff')),
}
SIDES = pytest.mark.parametrize('side', build.SIDE_LIBRARIES, ids=lambda s: s.name)


def _record(side):
    return {r.file: r for r in nat.LIBRARIES}[os.path.basename(side.out)]


def _names(side):
    """The module-level names of one library: ``(sources, headers, out, stale, build)`` of build.py, ``(name, path, version, exports,
    load, check)`` of _native.py."""
    upper, lower, out = EXPECT[side.name]['names']
    b = tuple(getattr(build, n) for n in (upper + '_SOURCES', upper + '_HEADERS', upper + '_' + out, lower + '_stale', 'build_' + lower))
    n = tuple(getattr(nat, n) for n in (upper + '_LIB_NAME', upper + '_LIB_PATH', upper + '_ABI_VERSION', upper + '_EXPORTS', 'load_' + lower,
                                        'check_' + lower))
    return b, n


def _every_other_list(side):
    """Every file any other library is made of, the first library included."""
    return set(build.SOURCES) | set(build.HEADERS) | {f for o in build.SIDE_LIBRARIES if o is not side for f in o.sources + o.headers}


@pytest.fixture(scope='module')
def built():
    return build.build(verbose=False)


def test_the_table_is_the_six_libraries_in_build_order(built):
    assert [s.name for s in build.SIDE_LIBRARIES] == list(EXPECT) == ['analysis', 'eval', 'locate', 'components', 'refine', 'selfaff']
    assert [r.file for r in nat.LIBRARIES] == ['libdaam_hip.so'] + [e['basename'] for e in EXPECT.values()]
    assert built == build.OUT and os.path.exists(built) and not build.stale()


@SIDES
def test_library_is_built_by_the_table_under_the_names_it_had(built, side):
    want = EXPECT[side.name]
    (sources, headers, out, stale, rebuild), (name, path, _, _, _, _) = _names(side)
    assert sources is side.sources and headers is side.headers and out == side.out and name == want['basename'] == os.path.basename(out)
    assert os.path.exists(out) and not stale() and not build.side_stale(side) and rebuild(verbose=False) == out
    assert all(os.path.exists(os.path.join(build.HERE, 'csrc', f)) for f in sources + headers)
    assert _record(side).env == want['env'] and (path == out or os.environ.get(want['env']))


@SIDES
def test_its_files_are_in_no_other_librarys_lists(side):
    want = EXPECT[side.name]
    mine = set(side.sources) | {os.path.join('..', '..', 'include', want['header'])} | set(want['own'])
    assert mine <= set(side.sources + side.headers)
    assert not mine & _every_other_list(side)


def test_the_lists_are_what_they_were():
    assert len(build.SOURCES) == 20 and len(build.HEADERS) == 25 and build.csrc_sha() == '75aa74ff4390'
    assert build.ANALYSIS_SOURCES == ['daam_key_scores.hip', 'daam_token_gram.hip', 'daam_key_blend.hip']
    assert build.EVAL_SOURCES == ['daam_threshold_sweep.hip'] and build.LOCATE_SOURCES == ['daam_locate.hip']
    assert build.COMPONENTS_SOURCES == ['daam_components.hip'] and build.REFINE_SOURCES == ['daam_refine.hip']
    assert build.SELFAFF_SOURCES == ['daam_self_affinity.hip']
    assert 'daam_refine.hip' not in build.SOURCES
    for side in build.SIDE_LIBRARIES:                      # no library's name in a list of another
        for frag in EXPECT[side.name]['fragments']:
            assert not [f for f in _every_other_list(side) if frag in f], (side.name, frag)


@SIDES
def test_exports_are_the_headers_and_the_bindings(built, side):
    want = EXPECT[side.name]
    _, (_, _, version, exports, load, _) = _names(side)
    rec = _record(side)
    names = LC.exported(side.out)
    assert names == LC.declared(want['header']) == sorted(exports) == sorted(rec.table) and len(names) == want['exports']
    lib = load()
    assert getattr(lib, rec.version_fn)() == want['abi'] == version == rec.abi_version
    assert {name: len(getattr(lib, name).argtypes) for name in want['argtypes']} == want['argtypes']


@SIDES
def test_header_is_c99(tmp_path, side):
    want = EXPECT[side.name]
    src = tmp_path / 'use.c'
    src.write_text('#include "%s"\nint main(void) { return %s == %d && sizeof(&%s) ? 0 : 1; }\n' % (want['header'], want['macro'], want['abi'], want['fn']))
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o',
                    str(tmp_path / 'use.o')], check=True)


@SIDES
def test_no_kernel_has_scratch(built, side):
    names = list(build.kernel_shas(side.out))
    assert len(names) == EXPECT[side.name]['kernels']
    LC.assert_no_scratch(side.out, names)


@SIDES
def test_deleted_library_is_rebuilt_alone(built, side):
    others = [build.OUT, build.fastpath_out()] + [o.out for o in build.SIDE_LIBRARIES if o is not side]
    stamps = [os.path.getmtime(p) for p in others]
    files = sorted(os.listdir(build.HERE))
    shas = build.kernel_shas(side.out)
    os.remove(side.out)
    assert not build.stale() and [build.side_stale(o) for o in build.SIDE_LIBRARIES] == [o is side for o in build.SIDE_LIBRARIES]
    build.build(verbose=False)
    assert os.path.exists(side.out) and not build.side_stale(side) and build.kernel_shas(side.out) == shas
    assert [os.path.getmtime(p) for p in others] == stamps
    assert sorted(os.listdir(build.HERE)) == files               # the build writes no other file


# ---- the recipe: every hipcc command, element for element, as build.py had it written out six times ------------------------------------
SIDE_FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-fvisibility=hidden']
SIDE_SOURCES = {
    'analysis': ['daam_key_scores.hip', 'daam_token_gram.hip', 'daam_key_blend.hip'], 'eval': ['daam_threshold_sweep.hip'],
    'locate': ['daam_locate.hip'], 'components': ['daam_components.hip'], 'refine': ['daam_refine.hip'], 'selfaff': ['daam_self_affinity.hip'],
}
MAIN_SOURCES = ['daam_api.hip', 'daam_tap_api.hip', 'daam_finalize_api.hip', 'daam_kernels.hip', 'daam_tap_mfma.hip', 'daam_tap_d64.hip',
                'daam_tap_wide.hip', 'daam_tap_chunk.hip', 'daam_tap_slab.hip', 'daam_tap_pair.hip', 'daam_tap_walk.hip', 'daam_attend_d64.hip',
                'daam_finalize.hip', 'daam_finalize_pipe.hip', 'daam_fin_bins.hip', 'daam_finalize_rect.hip', 'daam_epilogue.hip',
                'daam_word_masks.hip', 'daam_mask_matrix.hip', 'daam_region_scores.hip']


@pytest.fixture
def recorded(monkeypatch):
    """``build.subprocess.run`` records its argv and runs nothing."""
    calls = []

    def run(cmd, check):
        assert check is True
        calls.append(list(cmd))
    monkeypatch.setattr(build, 'subprocess', types.SimpleNamespace(run=run))
    return calls


def _csrc(f):
    return os.path.join(build.HERE, 'csrc', f)


def test_recorded_argv_of_the_side_libraries_and_a_variant(recorded):
    hipcc = build.hipcc()
    for side in build.SIDE_LIBRARIES:
        assert build.build_side(side, force=True, verbose=False) == side.out
    assert recorded == [[hipcc, *SIDE_FLAGS, *[_csrc(f) for f in SIDE_SOURCES[name]], '-o', os.path.join(build.HERE, EXPECT[name]['basename'])]
                        for name in EXPECT]
    del recorded[:]
    assert build.build_variant('x.so', ['-DX'], verbose=False) == 'x.so'
    assert recorded == [[hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-fvisibility=hidden', '-DX',
                         *[_csrc(f) for f in MAIN_SOURCES], '-o', 'x.so']]
    del recorded[:]
    for name in ('analysis', 'eval', 'locate', 'components', 'refine', 'self_affinity'):        # the kept names go the same way
        getattr(build, 'build_' + name)(True, False)
    assert [c[-1] for c in recorded] == [os.path.join(build.HERE, e['basename']) for e in EXPECT.values()]


def test_recorded_argv_of_the_whole_build(recorded, monkeypatch):
    monkeypatch.setattr(build, 'build_fastpath', lambda force, verbose: None)
    hipcc = build.hipcc()
    obj = lambda f: os.path.join(build.HERE, 'build', f + '.o')
    assert build.build(force=True, verbose=False) == build.OUT
    sides, compiles, link = recorded[:6], recorded[6:-1], recorded[-1]
    assert sides == [[hipcc, *SIDE_FLAGS, *[_csrc(f) for f in SIDE_SOURCES[name]], '-o', os.path.join(build.HERE, EXPECT[name]['basename'])]
                     for name in EXPECT]
    # the objects are compiled by a pool of threads: every line once, in any order, all of them before the link
    assert sorted(compiles) == sorted([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-c', _csrc(f), '-o', obj(f)]
                                      for f in MAIN_SOURCES) and len(compiles) == 20
    assert link == [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-fvisibility=hidden', *[obj(f) for f in MAIN_SOURCES], '-o',
                    os.path.join(build.HERE, 'libdaam_hip.so')]


# ---- the binding tables ----------------------------------------------------------------------------------------------------------------
BOUND = {'libdaam_hip.so': ('', 'EXPORTS'), 'libdaam_analysis.so': ('_analysis', 'ANALYSIS_EXPORTS'), 'libdaam_eval.so': ('_eval', 'EVAL_EXPORTS'),
         'libdaam_locate.so': ('_locate', 'LOCATE_EXPORTS'), 'libdaam_components.so': ('_components', 'COMPONENTS_EXPORTS'),
         'libdaam_refine.so': ('_refine', 'REFINE_EXPORTS'), 'libdaam_selfaff.so': ('_self_affinity', 'SELFAFF_EXPORTS')}
LIBS = pytest.mark.parametrize('rec', nat.LIBRARIES, ids=lambda r: r.file)


@LIBS
def test_every_export_has_a_table_row_and_carries_its_types(built, rec):
    suffix, exports = BOUND[rec.file]
    assert getattr(nat, exports) == tuple(rec.table) == rec.exports and len(set(rec.exports)) == len(rec.exports)
    assert rec.version_fn in rec.table and rec.error_fn in rec.table
    load = getattr(nat, 'load' + suffix)
    lib = load()
    assert load() is lib and lib._name == rec.path
    for name, (argtypes, restype) in rec.table.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes and fn.restype is restype, name
    assert rec.table[rec.error_fn] == (None, nat.c_char_p) and rec.table[rec.version_fn] == (None, nat.c_int)
    sized = [n for n in rec.table if n.endswith(('_workspace', '_bytes'))]
    assert all(rec.table[n][1] is nat.c_size_t for n in sized)
    assert all(rec.table[n][1] is nat.c_int for n in rec.table if n not in sized and n != rec.error_fn)
    if rec.file == 'libdaam_hip.so':                      # the only symbols without argument types are the two that take none
        assert [n for n, (a, _) in rec.table.items() if a is None] == ['daam_abi_version', 'daam_last_error'] and len(rec.table) == 44


@LIBS
def test_check_asks_the_loader_the_module_names_now(monkeypatch, rec):
    """``check_x`` reaches its library through ``nat.load_x`` at call time: a stand-in installed on the module is the one asked for the
    error text, and a return code of 0 asks nobody."""
    suffix, _ = BOUND[rec.file]
    text = ('said by the stand-in of ' + rec.file).encode()
    monkeypatch.setattr(nat, 'load' + suffix, lambda: types.SimpleNamespace(**{rec.error_fn: lambda: text}))
    check = getattr(nat, 'check' + suffix)
    with pytest.raises(nat.DaamError) as err:
        check(-1)
    assert err.value.code == -1 and text.decode() in str(err.value) and str(err.value) == 'libdaam_hip error -1: ' + text.decode()
    monkeypatch.setattr(nat, 'load' + suffix, lambda: pytest.fail('a passing call asked for the library'))
    assert check(0) is None
    monkeypatch.setattr(nat, 'load' + suffix, lambda: types.SimpleNamespace(**{rec.error_fn: lambda: None}))
    with pytest.raises(nat.DaamError, match=r'error -3: $'):
        check(-3)
