"""What the self-attention affinity and the joint tap share (daam_amd/csrc/daam_rowsoftmax32.h) moved no machine code:
every kernel of ``libdaam_selfaff.so`` and ``libdaam_joint.so`` has the fingerprint recorded for the parent commit
(profiles/rowsoftmax_refactor.json) and the one its own pull request recorded, the exports and the lists of the first library are what
they were, and every shared piece is defined once -- or, where no function form kept the bytes, exactly twice."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'daam_amd', 'csrc')
HEADER = 'daam_rowsoftmax32.h'
FILES = ('daam_self_affinity.hip', 'daam_joint_tap.hip', HEADER)


def _profile(name):
    return json.load(open(os.path.join(ROOT, 'profiles', name)))


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    return {'selfaff': build.build_self_affinity(verbose=False), 'joint': build.build_joint(verbose=False)}


def test_every_kernel_has_the_parent_builds_fingerprint(built):
    from daam_amd import build
    rec = _profile('rowsoftmax_refactor.json')
    assert rec['kernel_shas_equal'] is True and rec['kernel_count'] == {'selfaff': 29, 'joint': 8}
    assert rec['kernel_shas'] == rec['parent_kernel_shas'] and sorted(rec['kernel_shas']) == ['joint', 'selfaff']
    for name, lib in built.items():
        assert build.kernel_shas(lib) == rec['kernel_shas'][name] and len(rec['kernel_shas'][name]) == rec['kernel_count'][name], name


def test_the_fingerprints_their_own_profiles_recorded_still_hold(built):
    from daam_amd import build
    rec = _profile('rowsoftmax_refactor.json')
    assert rec['parent_matches_committed_profiles'] == {'profiles/self_affinity.json': True, 'profiles/joint_tap.json': True}
    for name, profile in (('selfaff', 'self_affinity.json'), ('joint', 'joint_tap.json')):
        pinned = _profile(profile)['kernel_shas']
        assert pinned == rec['kernel_shas'][name] == build.kernel_shas(built[name]), name


def test_exports_and_lists_are_unchanged(built):
    from daam_amd import build
    rec = _profile('rowsoftmax_refactor.json')
    assert rec['exported_symbols_equal'] is True
    for name, lib in built.items():
        nm = subprocess.run(['nm', '-D', '--defined-only', lib], capture_output=True, text=True, check=True).stdout
        assert sorted(re.findall(r' T (daam_\w+)$', nm, flags=re.M)) == rec['exported_symbols'][name], name
    assert len(rec['exported_symbols']['selfaff']) == 6 and len(rec['exported_symbols']['joint']) == 4
    assert build.csrc_sha() == '75aa74ff4390'
    assert HEADER in build.SELFAFF_HEADERS and HEADER in build.JOINT_HEADERS and HEADER not in build.HEADERS
    assert os.path.exists(os.path.join(CSRC, HEADER))
    users = [f for f in sorted(os.listdir(CSRC)) if HEADER in open(os.path.join(CSRC, f), errors='replace').read() and f != HEADER]
    assert users == ['daam_joint_tap.hip', 'daam_self_affinity.hip']
    text = open(os.path.join(CSRC, HEADER)).read()
    assert re.findall(r'#include "([^"]+)"', text) == ['../../include/daam_hip.h']


def _count(pattern):
    """{file name: occurrences of the literal text} over the three files, for those that hold it"""
    out = {}
    for f in FILES:
        n = open(os.path.join(CSRC, f)).read().count(pattern)
        if n:
            out[f] = n
    return out


def test_shared_pieces_are_defined_once():
    once = {HEADER: 1}
    assert _count('__builtin_amdgcn_mfma_f32_32x32x16_f16') == once and _count('__builtin_amdgcn_mfma_f32_32x32x16_bf16') == once
    assert _count('(reg & 3) + 8 * (reg >> 2) + 4 * half') == once                       # acc_row
    assert _count('1.4426950408889634') == once and _count('vsnprintf') == once and _count('thread_local') == once
    assert _count('hipGetLastError') == once and _count('ext_vector_type(16)') == once
    assert _count('__fmaf_rn(weight, acc') == once                                       # store_weighted
    assert _count(', c, st.x)), st.y, acc)') == once                                     # add_prob
    for message in ('DAAM_F16 or DAAM_BF16', 'at most %d slices', 'finite and > 0', 'is not finite', 'sums are not 4-byte aligned',
                    'the workspace is not 8-byte aligned', 'a multiple of 8 elements', 'slices of %d rows need'):
        assert _count(message) == once, message
    # Left at their call sites, once in either file: every function form of the 32-key online update and of the merge of the lane
    # halves rescheduled the statistics kernels ("trials" of profiles/rowsoftmax_refactor.json, the entries with "made": false).
    twice = {'daam_self_affinity.hip': 1, 'daam_joint_tap.hip': 1}
    assert _count('const float carry = m > -INFINITY ? __builtin_amdgcn_exp2f(negm_new - negm) : 0.f;') == twice
    assert _count('l = l * carry + part;') == twice
    assert _count('const float m_all = fmaxf(m_lo, m_hi);') == twice
    assert _count('make_float2(negm_all, 1.0f / (t_lo + t_hi))') == twice
    rec = _profile('rowsoftmax_refactor.json')
    assert len(rec['left_at_call_sites']) == 2 and sum(not t['made'] for t in rec['trials']) >= 2
    # ... and it is the same text in both, line for line
    sa, jt = (open(os.path.join(CSRC, f)).read() for f in FILES[:2])
    step = lambda s: s[s.index('const float m_new = fmaxf(m, top);'):s.index('negm = negm_new;')]
    merge = lambda s: re.sub(r' +// the lower half always holds (text )?key 0: finite', '', s[s.index('const float m_o = __shfl_xor'):s.index('1.0f / (t_lo + t_hi)')])
    assert step(sa) == step(jt) and merge(sa) == merge(jt)
