"""Discovery (include/daam_discover.h) without a GPU: ``libdaam_discover.so`` builds by the side libraries' recipe beside
their tables, exports what its header declares and what ``_native`` types; the header is C99; no kernel has scratch; every argument
the header rules out is refused before any HIP call; the float64 loop recovers planted partitions; the mutants leave the bounds; the
fixtures of the label pass keep the float64 reference inside its 1 % cap; and the Python layer (``SelfAffinity.discover``,
``Discovery``) on a numpy stand-in of the library.  The kernels run in ``test_gpu_discover.py``."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _discover_domain as DD
import _libcheck as LC
from oracle import fake_diffusers as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
KERNELS = ('discover_prepare_kernel', 'discover_pair_kl_kernel', 'discover_merge_kernel', 'discover_labels_kernel')
PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build_discover(verbose=False)
    return build.DISCOVER_LIB


@pytest.fixture(scope='module')
def lib(built):
    from daam_amd import _native as nat
    return nat.load_discover()


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_library_builds_and_exports_its_header(built, lib):
    from daam_amd import _native as nat, build
    assert os.path.exists(built) and os.path.basename(built) == 'libdaam_discover.so' and not build.discover_stale()
    assert build.DISCOVER_SOURCES == ['daam_discover.hip'] and build.DISCOVER.name == 'discover'
    exported = LC.exported(built)
    assert exported == LC.declared('daam_discover.h') == sorted(nat.DISCOVER_EXPORTS)
    assert exported == ['daam_discover_abi_version', 'daam_discover_labels', 'daam_discover_last_error', 'daam_discover_merge',
                        'daam_discover_pair_kl', 'daam_discover_prepare']
    assert lib.daam_discover_abi_version() == 1 == nat.DISCOVER_ABI_VERSION and nat.DISCOVER_LIBRARY.env == 'DAAM_DISCOVER_LIB'
    assert nat.load_discover.__name__ == 'load_discover' and nat.check_discover.__name__ == 'check_discover'
    names = list(build.kernel_shas(built))
    assert len(names) == 5 and all(any(k in n for k in KERNELS) for n in names) and sum('pair_kl' in n for n in names) == 2


def test_the_header_and_the_binding_agree_on_every_argument():
    """Every entry point of the header against ``_native``'s argtypes: the count, and pointer / int / int64 per position."""
    import ctypes
    from daam_amd import _native as nat
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'daam_discover.h')).read(), flags=re.S)
    seen = {}
    for ret, name, args in re.findall(r'DAAM_API ([\w \*]+?)\s*(daam_\w+)\(([^)]*)\);', text):
        seen[name] = [a.strip() for a in args.split(',') if a.strip() != 'void']
    assert sorted(seen) == sorted(nat.DISCOVER_EXPORTS)
    for name, args in seen.items():
        argtypes, restype = nat.DISCOVER_LIBRARY.table[name]
        assert (argtypes or []) == [ctypes.c_void_p if '*' in a else ctypes.c_int64 if a.startswith('int64_t') else ctypes.c_int for a in args], name
        assert restype is (ctypes.c_char_p if name.endswith('last_error') else ctypes.c_int)


def test_the_record_stands_outside_the_tables():
    from daam_amd import _native as nat, build
    assert [lib.name for lib in build.SIDE_LIBRARIES] == ['analysis', 'eval', 'locate', 'components', 'refine', 'selfaff']
    assert build.DISCOVER not in build.SIDE_LIBRARIES and isinstance(build.DISCOVER, build.SideLibrary)
    assert build.DISCOVER not in (build.JOINT, build.ROPE, build.JOINT_AFFINITY)
    assert nat.DISCOVER_LIBRARY not in nat.LIBRARIES and len(nat.LIBRARIES) == 7 and isinstance(nat.DISCOVER_LIBRARY, nat.Library)
    assert 'daam_discover.hip' not in build.SOURCES and not any('discover' in h for h in build.HEADERS)
    assert build.discover_stale.func is build.side_stale and build.build_discover.func is build.build_side
    assert build.discover_stale.args == build.build_discover.args == (build.DISCOVER,)
    assert all(os.path.exists(os.path.join(build.HERE, 'csrc', h)) for h in build.DISCOVER_HEADERS)
    text = open(os.path.join(build.HERE, 'csrc', 'daam_discover.hip')).read()
    assert [line for line in text.splitlines() if line.startswith('#include "')] == ['#include "../../include/daam_discover.h"']
    assert 'atomic' not in text.replace('No atomics', '')


def test_build_discover_is_the_side_recipe(monkeypatch):
    from daam_amd import build
    ran = []
    monkeypatch.setattr(build.subprocess, 'run', lambda cmd, check: ran.append(cmd))
    assert build.build_discover(force=True, verbose=False) == build.DISCOVER_LIB
    src = os.path.join(build.HERE, 'csrc', 'daam_discover.hip')
    assert ran == [[build.hipcc(), *build.HIPCC_FLAGS, src, '-o', build.DISCOVER_LIB]]
    ran.clear()
    build.build(force=True, verbose=False)
    assert not any('discover' in ' '.join(cmd) for cmd in ran), 'build() makes the libraries of its tables alone'


def test_staleness_follows_the_sources(tmp_path, monkeypatch):
    from daam_amd import build
    out = tmp_path / 'libdaam_discover.so'
    rec = build.DISCOVER._replace(out=str(out))
    assert build.side_stale(rec), 'a missing file is stale'
    out.write_bytes(b'')
    newest = max(os.path.getmtime(os.path.join(build.HERE, 'csrc', f)) for f in rec.sources + rec.headers)
    os.utime(out, (newest + 10, newest + 10))
    assert not build.side_stale(rec)
    os.utime(out, (newest - 10, newest - 10))
    assert build.side_stale(rec), 'older than a source or a header'


def test_header_is_c99(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "daam_discover.h"\nint main(void) { return DAAM_DISCOVER_ABI_VERSION == 1 && '
                   'sizeof(&daam_discover_pair_kl) ? 0 : 1; }\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o',
                    str(tmp_path / 'use.o')], check=True)


def test_no_kernel_has_scratch(built):
    from daam_amd import build
    LC.assert_no_scratch(built, list(build.kernel_shas(built)))


# ---- argument checks: all of them before any HIP call, so they run here ---------------------------------------------------------------
A0, A1, A2, A3, A4, A5 = (0x1000000 * i for i in range(1, 7))     # fake addresses 16 MiB apart (nothing is dereferenced)


def _call(lib, fn, args):
    rc = getattr(lib, 'daam_discover_' + fn)(*args)
    return rc, lib.daam_discover_last_error().decode()


BAD = {
    'prepare R 0': ('prepare', (A0, 8, 0, 8, A1, A2, None), 'R 0'), 'prepare R 16385': ('prepare', (A0, 8, 16385, 8, A1, A2, None), 'R 16385'),
    'prepare N 0': ('prepare', (A0, 8, 4, 0, A1, A2, None), 'N 0'), 'prepare N 16385': ('prepare', (A0, 16385, 4, 16385, A1, A2, None), 'N 16385'),
    'prepare stride below N': ('prepare', (A0, 7, 4, 8, A1, A2, None), 'stride'), 'prepare NULL src': ('prepare', (None, 8, 4, 8, A1, A2, None), 'NULL'),
    'prepare NULL L': ('prepare', (A0, 8, 4, 8, A1, None, None), 'NULL'), 'prepare P off 4 bytes': ('prepare', (A0, 8, 4, 8, A1 + 2, A2, None), '4-byte'),
    'prepare src off 4 bytes': ('prepare', (A0 + 1, 8, 4, 8, A1, A2, None), '4-byte'), 'prepare P over src': ('prepare', (A0, 8, 4, 8, A0 + 64, A2, None), 'overlaps'),
    'prepare L over P': ('prepare', (A0, 8, 4, 8, A1, A1 + 64, None), 'overlaps'),
    'pair_kl A 0': ('pair_kl', (A0, A1, 0, A2, A3, 4, 8, A4, None), 'A 0'), 'pair_kl A 16385': ('pair_kl', (A0, A1, 16385, A2, A3, 4, 8, A4, None), 'A 16385'),
    'pair_kl B 0': ('pair_kl', (A0, A1, 4, A2, A3, 0, 8, A4, None), 'B 0'), 'pair_kl B 16385': ('pair_kl', (A0, A1, 4, A2, A3, 16385, 8, A4, None), 'B 16385'),
    'pair_kl N 0': ('pair_kl', (A0, A1, 4, A2, A3, 4, 0, A4, None), 'N 0'), 'pair_kl N 16385': ('pair_kl', (A0, A1, 4, A2, A3, 4, 16385, A4, None), 'N 16385'),
    'pair_kl NULL Lb': ('pair_kl', (A0, A1, 4, A2, None, 4, 8, A4, None), 'NULL'), 'pair_kl NULL D': ('pair_kl', (A0, A1, 4, A2, A3, 4, 8, None, None), 'NULL'),
    'pair_kl La off 4 bytes': ('pair_kl', (A0, A1 + 2, 4, A2, A3, 4, 8, A4, None), '4-byte'), 'pair_kl D over Pb': ('pair_kl', (A0, A1, 4, A2, A3, 4, 8, A2 + 32, None), 'overlaps'),
    'merge R 0': ('merge', (A0, 0, 8, A1, 2, A2, A3, None), 'R 0'), 'merge N 16385': ('merge', (A0, 4, 16385, A1, 2, A2, A3, None), 'N 16385'),
    'merge K 0': ('merge', (A0, 4, 8, A1, 0, A2, A3, None), 'K 0'), 'merge K 1025': ('merge', (A0, 4, 8, A1, 1025, A2, A3, None), 'K 1025'),
    'merge NULL member': ('merge', (A0, 4, 8, None, 2, A2, A3, None), 'NULL'), 'merge NULL cnt': ('merge', (A0, 4, 8, A1, 2, A2, None, None), 'NULL'),
    'merge cnt off 4 bytes': ('merge', (A0, 4, 8, A1, 2, A2, A3 + 1, None), '4-byte'), 'merge out over member': ('merge', (A0, 4, 8, A1, 2, A1 + 4, A3, None), 'overlaps'),
    'merge cnt inside out': ('merge', (A0, 4, 8, A1, 2, A2, A2 + 8, None), 'overlaps'),
    'labels K 0': ('labels', (A0, 0, 4, 4, 8, 8, A1, None, None), 'K 0'), 'labels K 256': ('labels', (A0, 256, 4, 4, 8, 8, A1, None, None), 'K 256'),
    'labels h 0': ('labels', (A0, 2, 0, 4, 8, 8, A1, None, None), 'grid'), 'labels w 129': ('labels', (A0, 2, 4, 129, 8, 8, A1, None, None), 'grid'),
    'labels out_h 0': ('labels', (A0, 2, 4, 4, 0, 8, A1, None, None), 'output'), 'labels out_w 2049': ('labels', (A0, 2, 4, 4, 8, 2049, A1, None, None), 'output'),
    'labels NULL props': ('labels', (None, 2, 4, 4, 8, 8, A1, None, None), 'NULL'), 'labels NULL labels': ('labels', (A0, 2, 4, 4, 8, 8, None, None, None), 'NULL'),
    'labels values off 4 bytes': ('labels', (A0, 2, 4, 4, 8, 8, A1, A2 + 2, None), '4-byte'), 'labels labels over props': ('labels', (A0, 2, 4, 4, 8, 8, A0 + 8, None, None), 'overlaps'),
    'labels values over labels': ('labels', (A0, 2, 4, 4, 8, 8, A1, A1 + 60, None), 'overlaps'),
}
# The inside of every limit.  A call that passes the checks would launch, so each carries ONE fault that the last check catches (an
# output over an input): that message shows that the limit under test let the call through.
INSIDE = {
    'prepare R 16384 N 1': ('prepare', (A0, 1, 16384, 1, A0, A2, None)), 'prepare N 16384 wide stride': ('prepare', (A0, 20000, 2, 16384, A0, A2, None)),
    'pair_kl A B N at the top': ('pair_kl', (A0, A1, 16384, A2, A3, 16384, 16384, A0, None)), 'pair_kl ones': ('pair_kl', (A0, A1, 1, A2, A3, 1, 1, A0, None)),
    'pair_kl Pb is Pa': ('pair_kl', (A0, A1, 4, A0, A1, 4, 8, A1, None)), 'merge K 1024 R 16384': ('merge', (A0, 16384, 1, A1, 1024, A0, A3, None)),
    'labels K 255 grid 128 out 2048': ('labels', (A0, 255, 128, 128, 2048, 2048, A0, None, None)), 'labels ones': ('labels', (A0, 1, 1, 1, 1, 1, A0, None, None)),
}


@pytest.mark.parametrize('what', sorted(BAD))
def test_out_of_range_is_refused_before_any_hip_call(lib, what):
    fn, args, word = BAD[what]
    rc, msg = _call(lib, fn, args)
    assert rc == E_INVALID and msg.startswith(f'discover_{fn}: ') and word in msg, (what, rc, msg)


@pytest.mark.parametrize('what', sorted(INSIDE))
def test_inside_every_limit_reaches_the_overlap_check(lib, what):
    fn, args = INSIDE[what]
    rc, msg = _call(lib, fn, args)
    assert rc == E_INVALID and msg.startswith(f'discover_{fn}: ') and 'overlaps' in msg, (what, rc, msg)


# ---- the float64 loop on planted affinities -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('segments,grid', DD.PLANTED, ids=[f'S{s}-{g[0]}x{g[1]}' for s, g in DD.PLANTED])
def test_float64_discover_recovers_the_planted_partition(segments, grid):
    sums, truth = DD.planted(segments, grid)
    matrices = []
    labels, props = DD.discover64(sums, grid, anchors=grid, threshold=DD.THRESHOLD, iterations=3, matrices=matrices)
    for d in matrices:                                       # a condition on the inputs, not a tolerance
        assert (np.abs(d - DD.THRESHOLD) > 0.01 * DD.THRESHOLD).all(), 'an entry of D lies within 1 % of the threshold'
    same = truth.reshape(-1)[:, None] == truth.reshape(-1)[None, :]
    assert matrices[0][same].max() < 0.01 and matrices[0][~same].min() > 2.0, 'within a segment well below 1.1, across well above'
    assert props.shape[0] == segments and labels.shape == grid and DD.same_partition(labels, truth)


# ---- bounds and mutants ----------------------------------------------------------------------------------------------------------------
def _f32_pair_kl(pa, la, pb, lb):
    """The kernel's operation order in f32: subtractions and fma per term, j ascending."""
    acc = np.zeros((pa.shape[0], pb.shape[0]), np.float32)
    for j in range(pa.shape[1]):
        dp = (pa[:, None, j] - pb[None, :, j]).astype(np.float32)
        dl = (la[:, None, j] - lb[None, :, j]).astype(np.float32)
        acc = (dp.astype(np.float64) * dl.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return np.float32(0.5) * acc


@pytest.mark.parametrize('case', [c for c in DD.PAIR_CASES if c[2] <= 257], ids=DD.case_id)
def test_the_f32_order_is_inside_the_pair_kl_bound(case):
    pa, la, pb, lb = DD.pair_inputs(case)
    got, want, bound = _f32_pair_kl(pa, la, pb, lb), DD.pair_kl64(pa, la, pb, lb), DD.pair_kl_bound(pa, la, pb, lb)
    assert (np.abs(got - want) <= bound).all() and (want >= 0).all()
    if case[3] == 'self':
        assert (np.diag(got) == 0).all() and np.array_equal(got, got.T)
    if case[3] == 'near':
        assert 1e-9 < want.max() < 1e-5 and (bound <= 1e-3 * np.maximum(want, 1e-12) + 2.0 ** -125).all(), 'the bound resolves D ~ 1e-6'
    if case[3] == 'disjoint' and case[2] > 1:
        assert want.min() > 0.4 * -DD.LN_EPS


def _shows(mutant, case):
    a, b, n, regime = case
    if mutant == 'no_half':
        return n > 1 and (regime != 'self' or a > 1)           # one cell: every row is (1), D = 0
    if mutant == 'one_sided':                                  # with disjoint supports of equal mass KL(a|b) = KL(b|a) = D
        return regime == 'smooth' and n > 1
    if mutant == 'neighbour_L':                                # rows of one support share their logarithms' pattern
        return a > 1 and n > 1 and regime == 'smooth'
    return a > 1 and b > 1 and regime == 'smooth'              # past_N


@pytest.mark.parametrize('mutant', ['one_sided', 'no_half', 'neighbour_L', 'past_N'])
def test_pair_kl_mutants_leave_the_bound(mutant):
    cases = [c for c in DD.PAIR_CASES if _shows(mutant, c)]
    assert cases, mutant
    for case in cases:
        pa, la, pb, lb = DD.pair_inputs(case)
        want, bound = DD.pair_kl64(pa, la, pb, lb), DD.pair_kl_bound(pa, la, pb, lb)
        worst = float((np.abs(DD.pair_kl_mutant(pa, la, pb, lb, mutant) - want) / bound).max())
        assert worst > 50, (mutant, DD.case_id(case), worst)


def test_without_the_clamp_a_zero_cell_gives_nan():
    src = np.array([[1.0, 0.0, 3.0], [2.0, 2.0, 0.0]])
    p, l = DD.prepare64(src)
    assert np.isfinite(l).all() and l[0, 1] == DD.LN_EPS and np.isfinite(DD.pair_kl64(p, l, p, l)).all()
    p, l = DD.prepare64(src, eps=None)
    with np.errstate(invalid='ignore'):
        d = DD.pair_kl64(p, l, p, l)
    assert np.isnan(d).any() and not (np.abs(d - 0) <= DD.pair_kl_bound(*DD.prepare64(src) * 2)).all()


@pytest.mark.parametrize('case', DD.PREPARE_CASES, ids=DD.case_id)
def test_prepare_reference_and_bound(case):
    buf, stride = DD.prepare_inputs(case)
    src = buf[:, :case[1]]
    p, l = DD.prepare64(src)
    bp, bl = DD.prepare_bounds(src)
    assert np.isfinite(p).all() and np.isfinite(l).all() and (l >= DD.LN_EPS).all() and (l <= 0).all()
    live = src.sum(axis=1) != 0
    assert np.allclose(p[live].sum(axis=1), 1, rtol=1e-12) and (p[~live] == 0).all() and (l[~live] == DD.LN_EPS).all()
    # f32 in another order of addition stays inside the bound, a row sum that is off by one part in 1e4 does not
    p32 = (src / src.sum(axis=1, keepdims=True, dtype=np.float32).astype(np.float32)).astype(np.float32) if live.all() else None
    if p32 is not None:
        assert (np.abs(p32 - p) <= bp).all()
        assert not (np.abs(p * (1 + 1e-4) - p) <= bp).all() and (bl <= 1e-4).all()


@pytest.mark.parametrize('case', DD.MERGE_CASES, ids=DD.case_id)
def test_merge_reference_bound_and_mutants(case):
    k, r, n = case
    p, member = DD.merge_inputs(case)
    want, cnt = DD.merge64(p, member)
    bound = DD.merge_bound(p, member)
    assert want.shape == (k, n) and cnt.tolist() == [(member[i] != 0).sum() for i in range(k)]
    if k > 1:
        assert cnt[0] == 0 and (want[0] == 0).all() and cnt[1] == r and np.allclose(want[1], p.astype(np.float64).mean(axis=0))
    if k > 2:
        assert cnt[2] == 1 and np.array_equal(want[2], p[r // 2].astype(np.float64))
    f32 = np.zeros((k, n), np.float32)
    for i in range(k):
        for row in np.flatnonzero(member[i]):
            f32[i] += p[row]
        f32[i] /= np.float32(max(cnt[i], 1))
    assert (np.abs(f32 - want) <= bound).all()
    if r > 1 and k > 1:
        for mutant in ('transposed', 'mean_over_R'):
            worst = float((np.abs(DD.merge_mutant(p, member, mutant) - want) / bound).max())
            assert worst > 50, (mutant, case, worst)


@pytest.mark.parametrize('case', DD.LABEL_CASES, ids=DD.case_id)
def test_label_fixtures_stay_inside_the_cap_and_show_the_mutants(case):
    k, (h, w), (out_h, out_w), kind = case
    props = DD.label_inputs(case)
    labels, values, decided = DD.labels64(props, out_h, out_w)
    assert labels.shape == values.shape == decided.shape == (out_h, out_w)
    assert (~decided).sum() <= 0.01 * out_h * out_w, 'the float64 reference leaves out more than 1 % of the pixels'
    if (out_h, out_w) == (h, w):
        assert np.array_equal(labels, props.argmax(axis=0)) and np.array_equal(values, props.max(axis=0).astype(np.float64))
    if k > 1 and (out_h, out_w) != (h, w) and kind == 'smooth':
        other = DD.labels64(props, out_h, out_w, align_corners=True)[0]
        assert (other != labels)[decided].any(), 'align_corners=True decides differently where the margin is clear'


def test_a_tie_goes_to_the_lowest_index():
    props = DD.label_inputs((7, (5, 7), (5, 7), 'plateaus'))
    props = np.concatenate([props, props])                    # every proposal twice: exact ties everywhere
    low, high = DD.labels64(props, 10, 14)[0], DD.labels64(props, 10, 14, highest=True)[0]
    assert (low < 7).all() and np.array_equal(high, low + 7)


# ---- host side of discover -------------------------------------------------------------------------------------------------------------
def test_anchor_placement():
    from daam_amd.heatmap import discover_anchors
    assert discover_anchors((5, 7), (2, 3)) == [8, 10, 12, 22, 24, 26]            # rows 1, 3; columns 1, 3, 5
    assert discover_anchors((4, 4), 2) == [5, 7, 13, 15]
    assert discover_anchors((9, 13), (9, 13)) == list(range(117)), 'one anchor per cell'
    assert discover_anchors((2, 3), 4) == [0, 1, 1, 2, 0, 1, 1, 2, 3, 4, 4, 5, 3, 4, 4, 5], 'more anchors than cells: clipped, repeated'
    for grid in ((5, 7), (64, 64), (6, 10)):
        for anchors in (1, 3, 16, (2, 5)):
            assert discover_anchors(grid, anchors) == DD.anchors_of(grid, anchors)
    for bad in (0, (0, 3), (2, -1)):
        with pytest.raises(ValueError, match='anchors'):
            discover_anchors((4, 4), bad)


def test_the_greedy_pass_on_a_hand_written_matrix():
    from daam_amd.heatmap import discover_groups
    d = [[0.0, 0.5, 3.0, 1.0, 3.0],
         [0.5, 0.0, 3.0, 3.0, 0.2],
         [3.0, 3.0, 0.0, 3.0, 1.0],
         [1.0, 3.0, 3.0, 0.0, 3.0],
         [3.0, 0.2, 1.0, 3.0, 0.0]]
    # 0 takes 1 and 3 (list order, against the FIRST member only: 4 is close to 1 but not to 0); 2 takes 4
    assert discover_groups(d, 1.1) == [[0, 1, 3], [2, 4]] == DD.greedy(d, 1.1)
    assert discover_groups(torch.tensor(d), 1.0) == [[0, 1], [2], [3], [4]], 'the comparison is strict'
    assert discover_groups(d, 0.1) == [[0], [1], [2], [3], [4]] and discover_groups(d, 10) == [[0, 1, 2, 3, 4]]
    assert discover_groups([[0.0]], 1.1) == [[0]]


@pytest.fixture
def fakes(monkeypatch):
    return DD.install(monkeypatch.setattr)


def test_discover_on_the_stand_in_recovers_the_partitions(fakes):
    import daam_amd
    E, lib, loads = fakes
    for segments, grid in ((2, (4, 4)), (3, (5, 7)), (5, (9, 13))):
        sums, truth = DD.planted(segments, grid)
        aff = daam_amd.SelfAffinity(torch.from_numpy(sums), grid, 1, 1)
        assert not loads or lib.calls
        found = aff.discover(anchors=grid, threshold=DD.THRESHOLD, iterations=3)
        assert isinstance(found, daam_amd.Discovery) and found.n == segments and found.proposals.shape == (segments, *grid)
        assert found.labels.dtype == torch.uint8 and DD.same_partition(found.labels.numpy(), truth)
        want, _ = DD.discover64(sums, grid, anchors=grid, threshold=DD.THRESHOLD, iterations=3)
        assert np.array_equal(found.labels.numpy(), want)
        assert found.areas.dtype == torch.int64 and found.areas.tolist() == np.bincount(truth.reshape(-1)).tolist()
        assert found.masks.dtype == torch.uint8 and found.masks.shape == (segments, *grid) and (found.masks.sum(0) == 1).all()
        assert torch.equal(found.mask(1), found.masks[1]) and found.cpu().n == segments
        big = aff.discover(anchors=grid, threshold=DD.THRESHOLD, iterations=3, size=(2 * grid[0], 3 * grid[1]))
        assert big.labels.shape == (2 * grid[0], 3 * grid[1]) and big.n == segments

        class _Image:
            size = (31, 17)
        assert aff.discover(anchors=grid, iterations=2, size=_Image()).labels.shape == (17, 31), 'an image gives (W, H)'
    names = [c[0] for c in lib.calls[:9]]
    assert names == ['prepare', 'pair_kl', 'merge', 'prepare', 'pair_kl', 'merge', 'prepare', 'pair_kl', 'merge'] and lib.calls[9][0] == 'labels'


def test_every_value_error_of_discover(fakes):
    import daam_amd
    E, lib, loads = fakes
    sums, _ = DD.planted(2, (16, 16))
    aff = daam_amd.SelfAffinity(torch.from_numpy(sums), (16, 16), 1, 1)
    for kw, word in ((dict(threshold=0), 'threshold'), (dict(threshold=-1.0), 'threshold'), (dict(threshold=float('nan')), 'threshold'),
                     (dict(iterations=0), 'iterations'), (dict(anchors=0), 'anchors'), (dict(anchors=(2, 0)), 'anchors'),
                     (dict(size=(0, 4)), 'size'), (dict(size=(4, 2049)), 'size'), (dict(anchors=33), 'anchors')):
        with pytest.raises(ValueError, match=word):
            aff.discover(**kw)
    assert not lib.calls and not loads, 'all of them before any native call'
    with pytest.raises(ValueError, match='256 proposals are left'):
        aff.discover(anchors=16, iterations=1)               # one proposal per anchor
    with pytest.raises(ValueError, match='256 proposals are left'):
        aff.discover(anchors=16, threshold=1e-9, iterations=3)   # nothing merges
    assert aff.discover(anchors=16, iterations=2).n == 2


def test_the_launchers_check_shapes_and_dtypes_before_the_native_call(fakes):
    E, lib, loads = fakes
    f = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype)
    for call in (lambda: E.discover_prepare(f(4, 8, dtype=torch.float64)), lambda: E.discover_prepare(f(8)), lambda: E.discover_prepare(f(8, 4).t()),
                 lambda: E.discover_prepare(f(4, 8), out=(f(4, 8), f(4, 7))), lambda: E.discover_pair_kl(f(4, 8), f(4, 8), f(3, 7), f(3, 7)),
                 lambda: E.discover_pair_kl(f(4, 8), f(3, 8), f(3, 8), f(3, 8)), lambda: E.discover_pair_kl(f(4, 8), f(4, 8), f(3, 8), f(3, 8), out=f(3, 4)),
                 lambda: E.discover_pair_kl(f(4, 8), f(4, 8), f(3, 8, dtype=torch.float16), f(3, 8)), lambda: E.discover_merge(f(4, 8), f(2, 4)),
                 lambda: E.discover_merge(f(4, 8), f(2, 5, dtype=torch.uint8)), lambda: E.discover_merge(f(4, 8), f(1025, 4, dtype=torch.uint8)),
                 lambda: E.discover_labels(f(2, 4), 4, 4), lambda: E.discover_labels(f(256, 4, 4), 4, 4), lambda: E.discover_labels(f(2, 129, 4), 4, 4),
                 lambda: E.discover_labels(f(2, 4, 4), 0, 4), lambda: E.discover_labels(f(2, 4, 4), 4, 2049)):
        with pytest.raises(ValueError):
            call()
    assert not lib.calls
    labels, values = E.discover_labels(torch.tensor([[[1.0, 0.0]], [[0.0, 2.0]]]), 1, 2, values=True)
    assert labels.tolist() == [[0, 1]] and values.tolist() == [[1.0, 2.0]]


def test_names_and_word_masks(fakes, monkeypatch):
    """A hand-built ``GlobalHeatMap`` whose word rows are the planted segments; ``attribute`` is the masked sum of the planes at the
    grid's own size (what ``engine.region_scores`` gives when the masks have the maps' size)."""
    import daam_amd
    from daam_amd.utils import compute_token_merge_indices
    E, lib, loads = fakes
    grid = (8, 8)
    sums, truth = DD.planted(3, grid)
    found = daam_amd.SelfAffinity(torch.from_numpy(sums), grid, 1, 1).discover(anchors=grid, threshold=DD.THRESHOLD)
    tok = fd.FakeTokenizer()
    words = ['monkey', 'bicycle', 'photo']
    maps = np.zeros((13, *grid), np.float32)
    for seg, word in enumerate(words[:2]):                    # 'photo' owns nothing; segment 2 has no word
        for i in compute_token_merge_indices(tok, PROMPT, word, None)[0]:
            maps[i] = truth == seg
    ghm = daam_amd.GlobalHeatMap(tok, PROMPT, torch.from_numpy(maps))

    def region_scores(heat, masks, map_hw=None):
        m = masks.float()
        return torch.einsum('mhw,thw->mt', m, heat), m.sum(dim=(1, 2)).int(), m
    monkeypatch.setattr(E, 'region_scores', region_scores)
    seg_of = [int(found.labels[truth == s][0]) for s in range(3)]
    names = found.names(ghm, words)
    assert [names[seg_of[0]], names[seg_of[1]], names[seg_of[2]]] == ['monkey', 'bicycle', None]
    wm = found.word_masks(ghm, words)
    assert wm.dtype == torch.uint8 and wm.shape == (3, *grid)
    assert np.array_equal(wm[0].numpy(), truth == 0) and np.array_equal(wm[1].numpy(), truth == 1) and not wm[2].any()
    with pytest.raises(ValueError, match='at least one word'):
        found.names(ghm, [])
    with pytest.raises(ValueError, match='segment 3'):
        found.mask(3)


def test_nothing_is_loaded_unless_discover_is_called(fakes):
    import daam_amd
    E, lib, loads = fakes
    sums, _ = DD.planted(2, (4, 4))
    aff = daam_amd.SelfAffinity(torch.from_numpy(sums), (4, 4), 1, 1)
    aff.matrix(), aff.of(1, 1), aff.cpu()
    assert not loads and not lib.calls
    aff.discover(anchors=2)
    assert loads and lib.calls


def test_the_committed_profile_was_measured_on_these_kernels(built):
    import json
    from daam_amd import build
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'discover.json')))
    assert rec['kernel_shas'] == build.kernel_shas(built) and len(rec['kernel_shas']) == 5
    assert rec['bar']['met'] is True and [r['shape'] for r in rec['results']] == ['anchors_vs_cells', 'proposals_vs_proposals', 'discover_64x64_to_1024']
    legs = {'pair_kl': 'torch_pair_kl', 'discover': 'torch_discover'}
    assert all(r['ms'][r['leg']]['median'] <= r['ms'][legs[r['leg']]]['median'] for r in rec['results'])
