"""The joint affinity (include/daam_joint_affinity.h) without a GPU: ``libdaam_jointaff.so`` builds by the side libraries'
recipe beside their tables, exports what its header declares and the binding names; the header is C99; no kernel has scratch; every
argument the header rules out is refused before any HIP call; the f32 emulation is inside the bound and the mutants are outside it;
and the Python layer (``trace_joint`` / ``trace_flux`` with ``self_affinity=True``, ``engine.JointAffinityState``) on numpy stand-ins
of the two libraries.  The kernel runs in ``test_gpu_joint_affinity.py``."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import _flux_standin as FS
import _joint_affinity_domain as JA
import _libcheck as LC
import _mmdit_standin as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID = -1
N_KERNELS = 4                       # the image kernel for 2 dtypes x 2 head dims
PROMPT = 'A photo of a Monkey riding a bicycle and a monkey'


@pytest.fixture(scope='module')
def built():
    from daam_amd import build
    build.build_joint_affinity(verbose=False)
    return build.JOINT_AFFINITY_LIB


@pytest.fixture(scope='module')
def lib(built):
    from daam_amd import _native as nat
    return nat.load_joint_affinity()


# ---- the library -----------------------------------------------------------------------------------------------------------------------
def test_library_builds_and_exports_its_header(built, lib):
    from daam_amd import _native as nat, build
    assert os.path.exists(built) and os.path.basename(built) == 'libdaam_jointaff.so' and not build.joint_affinity_stale()
    assert build.JOINT_AFFINITY_SOURCES == ['daam_joint_affinity.hip'] and build.JOINT_AFFINITY.name == 'jointaff'
    exported = LC.exported(built)
    assert exported == LC.declared('daam_joint_affinity.h') == sorted(nat.JOINT_AFFINITY_EXPORTS)
    assert exported == ['daam_joint_affinity_abi_version', 'daam_joint_affinity_accumulate', 'daam_joint_affinity_last_error',
                        'daam_joint_affinity_stats_bytes']
    assert lib.daam_joint_affinity_abi_version() == 1 == nat.JOINT_AFFINITY_ABI_VERSION
    assert nat.JOINT_AFFINITY_LIBRARY.env == 'DAAM_JOINT_AFFINITY_LIB' and len(lib.daam_joint_affinity_accumulate.argtypes) == 21
    assert nat.load_joint_affinity.__name__ == 'load_joint_affinity' and nat.check_joint_affinity.__name__ == 'check_joint_affinity'
    names = list(build.kernel_shas(built))
    assert len(names) == N_KERNELS and all('joint_image_kernel' in n for n in names)


def test_the_record_stands_outside_the_tables():
    from daam_amd import _native as nat, build
    assert [lib.name for lib in build.SIDE_LIBRARIES] == ['analysis', 'eval', 'locate', 'components', 'refine', 'selfaff']
    assert build.JOINT_AFFINITY not in build.SIDE_LIBRARIES and isinstance(build.JOINT_AFFINITY, build.SideLibrary)
    assert build.JOINT_AFFINITY not in (build.JOINT, build.ROPE)
    assert nat.JOINT_AFFINITY_LIBRARY not in nat.LIBRARIES and len(nat.LIBRARIES) == 7 and isinstance(nat.JOINT_AFFINITY_LIBRARY, nat.Library)
    assert 'daam_joint_affinity.hip' not in build.SOURCES and not any('joint' in h for h in build.HEADERS)
    assert build.joint_affinity_stale.func is build.side_stale and build.build_joint_affinity.func is build.build_side
    assert build.joint_affinity_stale.args == build.build_joint_affinity.args == (build.JOINT_AFFINITY,)
    assert all(os.path.exists(os.path.join(build.HERE, 'csrc', h)) for h in build.JOINT_AFFINITY_HEADERS)
    # the source reads the two public headers and nothing of csrc/
    text = open(os.path.join(build.HERE, 'csrc', 'daam_joint_affinity.hip')).read()
    assert [line for line in text.splitlines() if line.startswith('#include "')] == ['#include "../../include/daam_joint_affinity.h"']


def test_build_joint_affinity_is_the_side_recipe(monkeypatch):
    from daam_amd import build
    ran = []
    monkeypatch.setattr(build.subprocess, 'run', lambda cmd, check: ran.append(cmd))
    assert build.build_joint_affinity(force=True, verbose=False) == build.JOINT_AFFINITY_LIB
    src = os.path.join(build.HERE, 'csrc', 'daam_joint_affinity.hip')
    assert ran == [[build.hipcc(), *build.HIPCC_FLAGS, src, '-o', build.JOINT_AFFINITY_LIB]]
    ran.clear()
    build.build(force=True, verbose=False)
    assert not any('joint' in ' '.join(cmd) for cmd in ran), 'build() makes the libraries of its tables alone'


def test_header_is_c99(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "daam_joint_affinity.h"\nint main(void) { return DAAM_JOINT_AFFINITY_ABI_VERSION == 1 && '
                   'sizeof(&daam_joint_affinity_accumulate) ? 0 : 1; }\n')
    subprocess.run(['cc', '-std=c99', '-pedantic', '-Wall', '-Werror', '-c', '-I', os.path.join(ROOT, 'include'), str(src), '-o',
                    str(tmp_path / 'use.o')], check=True)
    header = open(os.path.join(ROOT, 'include', 'daam_joint_affinity.h')).read()
    assert 's * pad128(P) + i' in header and 'Only rows i < P are read' in header, 'the header states the layout of the statistics itself'


def test_no_kernel_has_scratch(built):
    from daam_amd import build
    names = list(build.kernel_shas(built))
    LC.assert_no_scratch(built, names)
    kds = LC.kernel_descriptors(built)
    for k in names:
        group, = struct.unpack_from('<I', kds[k], 0)
        assert 0 < group <= 64 * 1024, (k, group)


def test_the_committed_profile_was_measured_on_these_kernels(built):
    import json
    from daam_amd import build
    rec = json.load(open(os.path.join(ROOT, 'profiles', 'joint_affinity.json')))
    assert rec['kernel_shas']['jointaff'] == build.kernel_shas(built) and len(rec['kernel_shas']['jointaff']) == N_KERNELS
    assert rec['bar']['met'] is True and [r['shape'] for r in rec['results']] == ['sd3_medium_1024', 'flux1_1024']
    assert all(r['affinity_cost_ms'] <= r['ms']['torch_affinity']['median'] for r in rec['results'])


# ---- argument checks: all of them before any HIP call, so they run here ---------------------------------------------------------------
ROW = 8 * 64


def _accumulate(lib, **over):
    """A call that is in range but for ``over``; pointers are small fake addresses (nothing is dereferenced)."""
    a = dict(q=0x100000, ki=0x300000, stats=0x2000000, stats_bytes=None, dtype=0, batch=2, heads=8, P=96, Pk=96, d=64, qs=(96 * ROW, 64, ROW),
             its=(96 * ROW, 64, ROW), scale=0.125, weight=1.0, accumulate=0, sums=0x1000000, stream=None)
    a.update(over)
    if a['stats_bytes'] is None:
        a['stats_bytes'] = lib.daam_joint_affinity_stats_bytes(a['batch'], a['heads'], a['P']) or 1 << 20
    rc = lib.daam_joint_affinity_accumulate(a['q'], a['ki'], a['stats'], a['stats_bytes'], a['dtype'], a['batch'], a['heads'], a['P'], a['Pk'],
                                            a['d'], *a['qs'], *a['its'], a['scale'], a['weight'], a['accumulate'], a['sums'], a['stream'])
    return rc, lib.daam_joint_affinity_last_error().decode()


BAD = {
    'f32 inputs': (dict(dtype=1), 'dtype'), 'batch 0': (dict(batch=0), 'slices'), 'heads 0': (dict(heads=0), 'slices'),
    '4097 slices': (dict(batch=4097, heads=1), 'slices'), 'P 0': (dict(P=0), 'P 0'), 'P 16385': (dict(P=16385), 'P 16385'),
    'Pk 0': (dict(Pk=0), 'Pk 0'), 'Pk 16385': (dict(Pk=16385), 'Pk 16385'), 'd 40': (dict(d=40), 'head dim 40'), 'd 160': (dict(d=160), 'head dim 160'),
    'd 0': (dict(d=0), 'head dim 0'), 'scale 0': (dict(scale=0.0), 'scale'), 'scale -1': (dict(scale=-1.0), 'scale'),
    'scale inf': (dict(scale=math.inf), 'scale'), 'scale nan': (dict(scale=math.nan), 'scale'), 'weight inf': (dict(weight=math.inf), 'weight'),
    'weight nan': (dict(weight=math.nan), 'weight'), 'NULL q': (dict(q=None), 'NULL'), 'NULL k_img': (dict(ki=None), 'NULL'),
    'NULL stats': (dict(stats=None), 'NULL'), 'NULL sums': (dict(sums=None), 'NULL'), 'q off 16 bytes': (dict(q=0x100008), '16-byte'),
    'k_img off 16 bytes': (dict(ki=0x300004), '16-byte'), 'stats off 8 bytes': (dict(stats=0x2000004), '8-byte'),
    'sums off 4 bytes': (dict(sums=0x1000002), '4-byte'), 'row stride not 8': (dict(qs=(96 * ROW, 64, ROW + 4)), 'stride'),
    'head stride not 8': (dict(its=(96 * ROW, 60, ROW)), 'stride'), 'negative stride': (dict(qs=(-8, 64, ROW)), 'stride'),
    'q row stride below d': (dict(qs=(96 * 32, 64, 32)), 'below the head dim'), 'k_img row stride below d': (dict(its=(96 * 32, 64, 32)), 'below the head dim'),
    'short stats': (dict(stats_bytes=8 * 16 * 128 - 8), 'stats of'), 'stats inside sums': (dict(stats=0x1000000 + 64), 'stats overlap sums'),
    'sums inside stats': (dict(sums=0x2000000 + 8 * 16 * 128 - 4), 'stats overlap sums'),
}
# The inside of every limit.  A call that passes the checks would launch, so each of these carries ONE fault that a later check
# catches (statistics eight bytes short): a message about them shows that the limit under test let the call through.
INSIDE = {
    'P 1': dict(P=1), 'P 16384': dict(P=16384), 'Pk 1': dict(Pk=1), 'Pk 16384': dict(Pk=16384), '4096 slices': dict(batch=64, heads=64),
    'one slice': dict(batch=1, heads=1), 'bf16': dict(dtype=2), 'd 128': dict(d=128, qs=(96 * 1024, 128, 1024), its=(96 * 1024, 128, 1024)),
    'packed layout': dict(qs=(8 * 96 * 64, 96 * 64, 64), its=(8 * 96 * 64, 96 * 64, 64)), 'zero batch stride': dict(its=(0, 64, ROW)),
    'tiny scale': dict(scale=1e-30), 'huge scale': dict(scale=1e30), 'weight 0': dict(weight=0.0), 'negative weight': dict(weight=-3.5),
    'accumulate 1': dict(accumulate=1), 'Pk not P': dict(Pk=200),
}


@pytest.mark.parametrize('what', sorted(BAD))
def test_out_of_range_is_refused_before_any_hip_call(lib, what):
    over, word = BAD[what]
    rc, msg = _accumulate(lib, **over)
    assert rc == E_INVALID and msg.startswith('joint_affinity_accumulate: ') and word in msg, (what, rc, msg)


@pytest.mark.parametrize('what', sorted(INSIDE))
def test_inside_every_limit_reaches_the_stats_check(lib, what):
    over = dict(INSIDE[what])
    shape = dict(batch=2, heads=8, P=96)
    shape.update({k: v for k, v in over.items() if k in shape})
    need = lib.daam_joint_affinity_stats_bytes(shape['batch'], shape['heads'], shape['P'])
    assert need > 0
    rc, msg = _accumulate(lib, **dict(over, stats_bytes=need - 8))
    assert rc == E_INVALID and msg.startswith('joint_affinity_accumulate: stats of'), (what, rc, msg)


def test_stats_bytes_are_those_of_the_joint_taps_workspace(lib):
    from daam_amd import _native as nat, build
    build.build_joint(verbose=False)
    tap, fake = nat.load_joint(), JA.FakeJointAffinityLib()
    for args in [(1, 1, 1), (2, 3, 128), (2, 3, 129), (64, 64, 16384), (1, 24, 4096), (0, 1, 5), (1, 0, 5), (65, 64, 5), (1, 1, 0), (1, 1, 16385)]:
        got = lib.daam_joint_affinity_stats_bytes(*args)
        assert got == tap.daam_joint_tap_workspace(*args) == fake.daam_joint_affinity_stats_bytes(*args), args
    assert lib.daam_joint_affinity_stats_bytes(2, 3, 129) == 8 * 6 * 256


# ---- reference, emulation, bound -------------------------------------------------------------------------------------------------------
def test_the_reference_is_the_image_block_of_one_softmax():
    q, kt, ki, scale = JA.inputs('small', 2, 3, 65, 77, 65, 64, 'f16', seed=1)
    calls = [(q, kt, ki, scale, 1.0)]
    aff = JA.reference_sums(calls)
    assert aff.shape == (65, 65)
    # a row sums to the slices minus the mass the cell gave to the text keys; with the text planes it is the whole softmax
    assert np.allclose(aff.sum(axis=1), 6 - JA.text_mass(calls), rtol=1e-13, atol=0)
    assert np.allclose(aff.sum(axis=1) + JA.J.reference_sums(calls).sum(axis=0), 6, rtol=1e-13, atol=0)
    assert (aff.sum(axis=1) < 6 - 0.5).all(), 'the text keys hold a clear share'
    assert np.allclose(JA.reference_sums([(0 * q, kt, ki, scale, 1.0)]), 6 / (77 + 65), rtol=1e-14, atol=0)
    two = JA.reference_sums([(q, kt, ki, scale, 0.5), (q, kt, ki, scale, -0.25)])
    assert np.allclose(two, 0.25 * aff, rtol=1e-13, atol=0)
    rect = JA.reference_sums([(q, kt, ki[:, :, :40], scale, 1.0)])
    assert rect.shape == (65, 40)


@pytest.mark.parametrize('case', JA.CASES, ids=[JA.case_id(c) for c in JA.CASES])
def test_the_emulation_is_inside_the_bound(case):
    for regime in dict.fromkeys((case[7], 'small')):
        q, kt, ki, scale = JA.case_inputs(case, regime)
        calls = [(q, kt, ki, scale, 1.0)]
        got, want, bound = JA.emulate_sums(calls), JA.reference_sums(calls), JA.sums_bound(calls)
        err = np.abs(got.astype(np.float64) - want)
        assert got.shape == want.shape == bound.shape == (case[0], case[2]) and np.isfinite(got).all() and (err <= bound).all(), float((err / bound).max())
        assert bound.max() <= 1e-2 * max(1.0, want.max()), 'the bound says something'


def _applies(mutant, case):
    P, T, Pk, d, dtype, (batch, heads), layout, regime = case
    if mutant == 'no_text_keys':
        return True
    if mutant == 'transposed':
        return P == Pk and P > 1
    if mutant == 'no_scale':
        return P > 1                                 # one image key beside the text keys still shows it; P = 1 with T = 1 need not
    if mutant == 'neighbour_stats':
        return P > 1
    if mutant == 'padded_row_stride':
        return Pk % 128 != 0 and P > 1
    return layout == 'interleaved' and heads > 1 and P > 1        # packed_head_stride


@pytest.mark.parametrize('mutant', JA.MUTANTS)
def test_mutants_fall_outside_the_bound(mutant):
    """Every mutant leaves the bound on EVERY listed shape it can show on, in the regime 'small' (where no probability is tiny)."""
    cases = [c for c in JA.CASES if _applies(mutant, c)]
    assert cases, mutant
    for case in cases:
        q, kt, ki, scale = JA.case_inputs(case, 'small')
        calls = [(q, kt, ki, scale, 1.0)]
        got, want, bound = JA.emulate_sums(calls, mutant=mutant), JA.reference_sums(calls), JA.sums_bound(calls)
        worst = float((np.abs(got.astype(np.float64) - want) / bound).max())
        assert worst > 50, (mutant, JA.case_id(case), worst)


def test_two_calls_chain_inside_the_bound():
    q1, kt1, ki1, scale = JA.inputs('small', 1, 3, 65, 77, 65, 64, 'f16', seed=1)
    q2, kt2, ki2, _ = JA.inputs('outlier', 1, 3, 65, 77, 65, 64, 'f16', seed=2)
    for w1, w2 in ((1.0, 1.0), (0.5, -0.25)):
        calls = [(q1, kt1, ki1, scale, w1), (q2, kt2, ki2, scale, w2)]
        got, want, bound = JA.emulate_sums(calls), JA.reference_sums(calls), JA.sums_bound(calls)
        assert (np.abs(got - want) <= bound).all() and (bound > JA.sums_bound(calls[:1])).all()


def test_the_block_case_gains_in_float64():
    """The seed of the block-structured case is chosen so that the float64 path itself shows the gain the device test asks for."""
    qk, kt, truth, plane = JA.block_case()
    h, w = JA.BLOCK_GRID
    assert qk.shape == (1, 1, h * w, 64) and kt.shape == (1, 1, JA.BLOCK_TEXT, 64) and 40 <= truth.sum() <= 100
    calls = [(qk, kt, qk, float(np.float32(64 ** -0.5)), 1.0)]
    norm = lambda m: (m - m.min()) / (m.max() - m.min())
    before = JA.iou(norm(plane) > 0.5, truth)
    after = JA.iou(norm(JA.propagate64(JA.reference_sums(calls), plane.reshape(1, -1), 2)[0].reshape(h, w)) > 0.5, truth)
    print(f'\nblock case 12 x 20 in float64: IoU {before:.3f} -> {after:.3f}; least text mass {JA.text_mass(calls).min():.3f}')
    assert before < 0.6 and after > before + 0.2 and after >= 0.9
    assert JA.text_mass(calls).min() > 1e-3, 'the text keys take a share of every row'


# ---- the Python layer on numpy stand-ins of the libraries ------------------------------------------------------------------------------
@pytest.fixture
def fakes(monkeypatch):
    return JA.install(monkeypatch.setattr)


def _follows(joint, aff, cells, heads, d):
    """Every affinity call follows its joint call: the same q / k_img pointers, that call's workspace as the statistics."""
    assert len(aff.calls) == len(joint.ptrs) == len(joint.calls)
    for (q, ki, ws), call, tap in zip(joint.ptrs, aff.calls, joint.calls):
        assert call[:3] == (q, ki, ws) and call[3] >= 8 * call[5] * call[6] * 128 * -(-cells // 128)
        assert call[4] == tap[0] and call[5:10] == (tap[1], tap[2], cells, cells, d) and call[6] == heads
        assert call[10] == tap[7][:3] + tap[7][6:] and call[11] == tap[8] and call[12] == 1.0
    assert [c[13] for c in aff.calls] == [0] + [1] * (len(aff.calls) - 1)


@pytest.mark.parametrize('batch', [2, 1])
def test_trace_joint_with_self_affinity(fakes, batch):
    import daam_amd
    E, joint, aff_lib, loads = fakes
    steps = 2
    pipe = M.make_pipe(seed=3, batch=batch)
    recorded = M.record(pipe)
    pipe(PROMPT, num_inference_steps=steps)
    plain = [o.clone() for o in pipe.outputs]
    M.record(pipe, on=False)
    with daam_amd.trace_joint(pipe) as tc:
        pipe(PROMPT, num_inference_steps=steps)
        off = tc.raw_heat_maps().clone()
        with pytest.raises(ValueError, match='self_affinity=True'):
            tc.compute_self_affinity()
    assert not loads and not aff_lib.calls and tc.affinity is None, 'with the option off nothing is loaded'
    joint.calls.clear()
    joint.ptrs.clear()
    with daam_amd.trace_joint(pipe, self_affinity=True) as tc:
        assert tc.affinity.sums is None and not loads, 'nothing is allocated or loaded before a call is tapped'
        with pytest.raises(RuntimeError, match='No affinity'):
            tc.compute_self_affinity()
        pipe(PROMPT, num_inference_steps=steps)
        assert all(torch.equal(a, b) for a, b in zip(plain, pipe.outputs)), 'the traced generation is bit-identical'
        assert torch.equal(tc.raw_heat_maps(), off), 'the heat-map planes do not see the option'
        aff = tc.compute_self_affinity()
        ghm = tc.compute_global_heat_map()
    kept = batch - batch // 2
    _follows(joint, aff_lib, 64, 2, 64)
    assert isinstance(aff, daam_amd.SelfAffinity) and aff.grid == (8, 8) and aff.calls == 3 * steps and aff.slices == 3 * steps * kept * 2
    calls = [(q, kt, ki, scale, 1.0) for q, kt, ki, scale in recorded]
    want, bound = JA.reference_sums(calls), JA.sums_bound(calls)
    assert (np.abs(aff.sums.numpy() - want) <= bound).all()
    assert np.allclose(aff.sums.numpy().sum(axis=1), aff.slices - JA.text_mass(calls), rtol=1e-5, atol=0), 'slices minus the text mass'
    assert torch.allclose(aff.matrix().sum(dim=1), torch.ones(64), atol=1e-5)
    assert ghm.heat_maps.shape == (77, 8, 8)
    # a second generation starts over
    with daam_amd.trace_joint(pipe, self_affinity=True) as tc:
        pipe(PROMPT, num_inference_steps=1)
        first = tc.compute_self_affinity()
        pipe(PROMPT, num_inference_steps=1)
        again = tc.compute_self_affinity()
    assert first.calls == again.calls == 3 and torch.equal(first.sums, again.sums) and first.sums is not again.sums


def _fake_rope(jobs, d):
    for x, out, cos, sin, heads in jobs:
        b, rows, ch = x.shape
        out.copy_(FS.apply_rotary(x.view(b, rows, heads, d).transpose(1, 2), cos, sin).transpose(1, 2).reshape(b, rows, ch))


@pytest.mark.parametrize('blocks,d', [('all', 64), ('double', 128), ('single', 64)])
def test_trace_flux_with_self_affinity(fakes, monkeypatch, blocks, d):
    import daam_amd
    E, joint, aff_lib, loads = fakes
    monkeypatch.setattr(E, 'rope_apply', _fake_rope)
    steps = 2
    pipe = FS.make_pipe(seed=2, dim_head=d)
    recorded = FS.record(pipe)
    pipe(PROMPT, num_inference_steps=steps)
    plain = [o.clone() for o in pipe.outputs]
    FS.record(pipe, on=False)
    with daam_amd.trace_flux(pipe, height=128, width=128, blocks=blocks) as tc:
        pipe(PROMPT, num_inference_steps=steps)
        off = tc.raw_heat_maps().clone()
        with pytest.raises(ValueError, match='self_affinity=True'):
            tc.compute_self_affinity()
    assert not loads and not aff_lib.calls, 'with the option off nothing is loaded'
    joint.calls.clear()
    joint.ptrs.clear()
    with daam_amd.trace_flux(pipe, height=128, width=128, blocks=blocks, self_affinity=True) as tc:
        pipe(PROMPT, num_inference_steps=steps)
        assert all(torch.equal(a, b) for a, b in zip(plain, pipe.outputs))
        assert torch.equal(tc.raw_heat_maps(), off)
        aff = tc.compute_self_affinity()
        kinds = tc.calls_by_kind()
    _follows(joint, aff_lib, 64, 2, d)
    calls = [(q, kt, ki, scale, 1.0) for kind, q, kt, ki, scale in recorded if blocks in ('all', kind)]
    assert aff.calls == len(calls) == sum(kinds.values()) == (4 if blocks == 'all' else 2) * steps and aff.slices == 2 * len(calls)
    # the rotated Q and K: the reference is fed what the model's own softmax saw
    want, bound = JA.reference_sums(calls), JA.sums_bound(calls)
    assert (np.abs(aff.sums.numpy() - want) <= bound).all()
    buf = tc._rotated
    assert all(buf.data_ptr() <= c[0] < buf.data_ptr() + buf.numel() * 2 for c in aff_lib.calls), 'q is read from the rotated buffer'


def test_joint_affinity_state_holds_its_limits(fakes):
    E, joint, aff_lib, loads = fakes
    for bad in (dict(h=0, w=4), dict(h=129, w=128)):
        with pytest.raises(ValueError):
            E.JointAffinityState(**bad)
    state = E.JointAffinityState(2, 3)
    x = lambda rows, ch=128, dt=torch.bfloat16: torch.zeros(1, rows, ch, dtype=dt)
    stats = torch.zeros(2 * 128, dtype=torch.int64)
    with pytest.raises(ValueError, match='square'):
        state.tap(x(6), x(5), 2, 0.125, stats)                               # 5 image keys on 6 cells
    with pytest.raises(ValueError, match='joint affinity tap'):
        state.tap(x(7), x(7), 2, 0.125, stats)
    with pytest.raises(ValueError, match='head dim'):
        state.tap(x(6), x(6), 4, 0.125, stats)
    with pytest.raises(RuntimeError, match='fp16 or bf16'):
        state.tap(x(6, dt=torch.float32), x(6, dt=torch.float32), 2, 0.125, stats)
    with pytest.raises(ValueError, match='statistics'):
        state.tap(x(6), x(6), 2, 0.125, stats[:100])
    with pytest.raises(ValueError, match='statistics'):
        state.tap(x(6), x(6), 2, 0.125, None)
    assert state.sums is None and not aff_lib.calls
    tap = E.JointTapState(2, 3, 5)
    assert tap.stats is None
    tap.tap(x(6), x(5), x(6), 2, 0.125)
    assert tap.stats is tap._ws and tap.stats.numel() * 8 == 8 * 2 * 128
    state.tap(x(6), x(6), 2, 0.125, tap.stats)                               # zero Q: 1 / (5 + 6) per slice and key
    assert state.calls == 1 and state.slices == 2 and torch.allclose(state.sums, torch.full((6, 6), 2 / 11))
    state.reset()
    assert state.calls == 0 and state.sums is not None


def test_the_first_load_checks_the_joint_taps_abi(fakes, monkeypatch):
    E, joint, aff_lib, loads = fakes
    monkeypatch.setattr(joint, 'daam_joint_tap_abi_version', lambda: 2, raising=False)
    with pytest.raises(RuntimeError, match='ABI 1'):
        E._load_joint_affinity()
    monkeypatch.setattr(joint, 'daam_joint_tap_abi_version', lambda: 1, raising=False)
    assert E._load_joint_affinity() is aff_lib and E._joint_affinity_checked
