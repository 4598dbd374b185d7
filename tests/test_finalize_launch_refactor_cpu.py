"""The finalize's device-facing text in one header and one launch idiom (daam_amd/csrc/daam_finalize.h) moved no machine
code: every kernel of the library has the fingerprint recorded for the parent commit (profiles/finalize_launch_refactor.json) and the
exports are the parent's.  What the header was made for holds in the source tree: no per-dtype launch ladder and no dtype literal in
the finalize sources, the shared helpers defined once, the finalize out of daam_kernels.hip / daam_ctx.h / daam_types.h, and one
host table behind every class kernel name ``daam_last_kernels`` reports."""
import glob
import json
import os
import re
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'daam_amd', 'csrc')
FIN_SOURCES = ('daam_finalize.hip', 'daam_finalize_pipe.hip', 'daam_finalize_rect.hip', 'daam_fin_bins.hip')
HEADER = 'daam_finalize.h'
# a launch text and the kernel it names (with the up kernels' S): fin_launch(kernel<...>, or the two older spellings
LAUNCH = re.compile(r'(?:fin_launch|hipLaunchKernelGGL|DAAM_LAUNCH)\(\(?\s*(\w+_kernel)(?:<\s*\w+\s*,\s*(\w+)\s*>)?')


def _src(name):
    return open(os.path.join(CSRC, name), errors='replace').read()


def _profile():
    return json.load(open(os.path.join(ROOT, 'profiles', 'finalize_launch_refactor.json')))


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    lib = build.build(verbose=False)
    return lib, build.kernel_shas(lib)


def test_every_kernel_has_the_parent_builds_fingerprint(built):
    _, have = built
    rec = _profile()
    assert rec['kernel_shas_equal'] is True and rec['kernel_count'] == {'parent': 191, 'new': 191}
    assert rec['kernel_shas'] == rec['parent_kernel_shas'] and len(rec['kernel_shas']) == 191
    assert {k: have.get(k) for k in rec['kernel_shas']} == rec['kernel_shas']
    assert len(have) == 191
    # the instantiation the dispatcher must not rename: the general kernel on __half, not _Float16
    assert any(k.startswith('_ZN4daam15finalize_kernelI6__halfEE') for k in have)
    assert 'cross-compiled' in rec['method'].lower()


def test_exports_are_the_parents(built):
    import subprocess
    from daam_amd import _native
    lib, _ = built
    rec = _profile()
    nm = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
    assert rec['exported_symbols_equal'] is True
    assert sorted(re.findall(r' T (daam_\w+)$', nm, flags=re.M)) == rec['exported_symbols']
    assert _native.load().daam_abi_version() == 6


def test_no_dtype_ladder_is_left():
    targets = Counter()
    for name in FIN_SOURCES:
        targets.update(LAUNCH.findall(_src(name)))
    assert targets, 'no launch text found: the pattern no longer matches the idiom'
    assert {k: n for k, n in targets.items() if n > 1} == {}     # (kernel, S): the up kernels once per S at most
    per_kernel = Counter(k for k, _ in targets.elements())
    assert {k: n for k, n in per_kernel.items() if n > (2 if k.startswith('finalize_up_') else 1)} == {}
    assert sum(targets.values()) < _profile()['launch_texts']['parent'] and _profile()['launch_texts']['new'] < _profile()['launch_texts']['parent']
    # every launch goes through the one function; the raw launch is written once, in it
    assert [n for n in FIN_SOURCES if 'hipLaunchKernelGGL' in _src(n)] == []
    assert _src(HEADER).count('hipLaunchKernelGGL(') == 1
    for name in FIN_SOURCES + (HEADER, 'daam_fin_rect.h', 'daam_fin_bins.h'):
        text = re.sub(r'//[^\n]*', '', _src(name))
        assert re.findall(r'dtype\s*[!=]=\s*\d', text) == [], name
        assert re.findall(r'\bdt\s*[!=]=\s*\d', text) == [], name
    assert len(re.findall(r'\bcase DAAM_(?:F16|BF16|F32):', _src(HEADER))) == 3
    assert 'same_grid(L, dtype, &gx, &gy)' in _src('daam_finalize.hip') and 'kPerPiece' in _src('daam_finalize.hip').split('same_grid(')[1]


def test_helpers_are_defined_once():
    text = {os.path.basename(p): open(p, errors='replace').read() for p in sorted(glob.glob(os.path.join(CSRC, '*')))}
    for pattern in (r'hipError_t allow_lds\(K kernel', r'float fin_max_nonneg\(float', r'hipError_t fin_dispatch\(int',
                    r'struct FinLaunch \{', r'float ld<__half>\(', r'void st<__half>\(', r'float round_to<__half>\('):
        assert sum(len(re.findall(pattern, t)) for t in text.values()) == 1, pattern
    where = [n for n, t in text.items() if 'pipe_max_nonneg' in t]
    not_made = ' '.join(h['piece'] for h in _profile()['hoists_not_made'])
    assert where == [] or 'pipe_max_nonneg' in not_made
    for vec in ('half8', 'floatx16', 'float4v', 'ushort8'):
        assert [n for n, t in text.items() if re.search(r'typedef [^;]*\b%s\b' % vec, t) and n.startswith(('daam_fin', 'daam_kernels'))] \
            == [HEADER], vec


def test_files_and_headers_hold_what_they_should():
    from daam_amd import build
    assert re.findall(r'finalize_\w*kernel|zero_groups', _src('daam_kernels.hip')) == []
    assert 'launch_finalize' not in _src('daam_ctx.h') and 'launch_zero_groups' not in _src('daam_ctx.h')
    assert re.findall(r'\bFin\w+', _src('daam_types.h')) == []
    for name in ('finalize_kernel', 'finalize_grouped_kernel', 'zero_groups_kernel'):
        assert re.search(r'__global__[^\n]*void %s\(' % name, _src('daam_finalize.hip')), name
    assert HEADER in build.HEADERS and 'daam_elem.h' in build.HEADERS
    assert all(os.path.exists(os.path.join(CSRC, f)) for f in build.SOURCES + build.HEADERS)
    for name in FIN_SOURCES + ('daam_finalize_api.hip',):
        seen, todo = set(), [name]
        while todo:                                              # the header reaches every finalize source, directly or not
            for inc in re.findall(r'#include "([\w.]+)"', _src(todo.pop())):
                if inc not in seen and os.path.exists(os.path.join(CSRC, inc)):
                    seen.add(inc)
                    todo.append(inc)
        assert HEADER in seen, name


def test_reported_kernel_names_come_from_one_table():
    api = _src('daam_finalize_api.hip')
    table = api.split('kFinClass[kFinClasses] = {')[1].split('};')[0]
    rows = re.findall(r'\{"(\w+)", "([^"]*)", (\w+)(?:<\d+>)?\}', table)
    assert [r[:2] for r in rows] == [('finalize_same', ''), ('finalize_up', '<32>'), ('finalize_up', '<16>'), ('finalize', ''),
                                     ('finalize_down2', '')]          # class 0 .. 4 (kFinClasses)
    # the one place a table row becomes a name
    assert api.count('(G ? "_grouped_kernel" : "_kernel")') == 1
    assert 'std::string(k.stem) + (G ? "_grouped_kernel" : "_kernel") + k.targ + "<" + dtype_name(dtype) + ">"' in api
    assert 'dt == DAAM_F32 ? "f32" : dt == DAAM_BF16 ? "bf16" : "f16"' in _src('daam_ctx.h')
    made = {stem + form + targ + '<' + dt + '>' for stem, targ, _ in rows for form in ('_kernel', '_grouped_kernel')
            for dt in ('f16', 'bf16', 'f32')}
    want = set()
    for dt in ('f16', 'bf16', 'f32'):
        for g in ('', '_grouped'):
            want |= {f'finalize_same{g}_kernel<{dt}>', f'finalize_up{g}_kernel<32><{dt}>', f'finalize_up{g}_kernel<16><{dt}>',
                     f'finalize{g}_kernel<{dt}>', f'finalize_down2{g}_kernel<{dt}>'}
    assert made == want and len(want) == 30
    # no class kernel is named anywhere else in the host file, and the special cases keep their literal names
    assert re.findall(r'"finalize(?:_same|_up|_down2)?(?:_grouped)?_kernel', api) == []
    for literal in ('"finalize_up32_pipe_kernel"', '"finalize_up32_pipe_grouped_kernel"', '"finalize_up32_same_kernel", "f16"',
                    '"finalize_up32_mfma_kernel", "f16"', '" + same-size keys"', '"finalize_rect_kernel" : "finalize_rect_grouped_kernel"',
                    '"finalize_bin_sum_kernel<"'):
        assert literal in api, literal
    # each launcher the table names is a class launcher of the header
    for _, _, fn in rows:
        assert re.search(r'\b%s\b' % fn, _src(HEADER)), fn


def test_less_text_than_the_parent():
    rec = _profile()['lines']
    files = rec['files']
    assert set(FIN_SOURCES) | {'daam_kernels.hip', 'daam_finalize_api.hip', 'daam_ctx.h', 'daam_types.h', HEADER, 'daam_elem.h',
                               'daam_fin_rect.h', 'daam_fin_bins.h'} == set(files)
    assert rec['new'] < rec['parent'] and rec['parent'] - rec['new'] == rec['fewer']
